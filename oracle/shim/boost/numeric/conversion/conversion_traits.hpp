// ORACLE — TEST INFRASTRUCTURE ONLY.  Stand-in for <boost/numeric/conversion/conversion_traits.hpp>, written for
// oracle/vdb_ref.cpp: OpenVDB's math headers use conversion_traits<T, S>::supertype only, the wider of two arithmetic types,
// which for the built-in types is std::common_type.
#ifndef ORACLE_SHIM_BOOST_CONVERSION_TRAITS_HPP
#define ORACLE_SHIM_BOOST_CONVERSION_TRAITS_HPP
#include <type_traits>

namespace boost {
namespace numeric {
template<typename T, typename S>
struct conversion_traits {
    typedef typename std::common_type<T, S>::type supertype;
};
}  // namespace numeric
}  // namespace boost
#endif
