// ORACLE — TEST INFRASTRUCTURE ONLY.  Stand-in for <boost/cstdint.hpp>, written for oracle/vdb_ref.cpp: the fixed-width
// integer types of <cstdint> under the names OpenVDB's headers expect in namespace boost.
#ifndef ORACLE_SHIM_BOOST_CSTDINT_HPP
#define ORACLE_SHIM_BOOST_CSTDINT_HPP
#include <cstdint>

namespace boost {
using std::int8_t;
using std::int16_t;
using std::int32_t;
using std::int64_t;
using std::uint8_t;
using std::uint16_t;
using std::uint32_t;
using std::uint64_t;
}  // namespace boost
#endif
