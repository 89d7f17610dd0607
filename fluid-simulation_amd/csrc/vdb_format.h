// What the two .vdb writers (vdb_writer.cpp: the density grid, every leaf of [lo,hi]^3; vdb_sdf_writer.cpp: the liquid surface,
// the listed leaves only) say about OpenVDB's file format 224 and its Tree_float_5_4_3, each thing once: the output stream and the
// zipToStream framing, the file header, everything of a grid in front of its tree, and the two records whose bytes do not depend
// on which leaves a tree has.  The library's sources are cited in vdb_writer.cpp's head comment.  Header only, like leaf_list.h.
#pragma once
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <ctime>
#include <random>
#include <string>
#include <vector>

#include "leaf_list.h"

namespace {

constexpr int INT1 = 128, INT2 = 4096;                       // Tree_float_5_4_3: 8^3 leaves (LEAF), 16^3 of them, 32^3 of those
constexpr uint32_t COMPRESS_ZIP = 0x1, COMPRESS_ACTIVE_MASK = 0x2;   // io/Compression.h:79-80
constexpr int8_t NO_MASK_OR_INACTIVE_VALS = 0;               // io/Compression.h:94

// zipToStream's framing of n bytes (io/Compression.cc:70-100: compress2 at Z_DEFAULT_COMPRESSION): the int64 that goes in front.
// Positive: that many compressed bytes follow, the first ones of z.  Otherwise zipping did not shrink them and it is -n: the raw
// bytes follow.  z only grows, so a caller that keeps it pays for its size once.
inline int64_t zip_frame(const void* p, size_t n, std::vector<unsigned char>& z)
{
    static const unsigned char none = 0;
    uLongf zn = compressBound((uLong)n);
    if (z.size() < zn) z.resize(zn);
    const int st = compress2(z.data(), &zn, n ? (const Bytef*)p : &none, (uLong)n, Z_DEFAULT_COMPRESSION);
    return st == Z_OK && zn < n ? (int64_t)zn : -(int64_t)n;
}

// buffered stream to the file (a 512^3 grid is 0.6 GB: nothing is held in memory); offsets are patched by seeking back
struct Out {
    FILE* f = nullptr;
    size_t at = 0;
    bool ok = true;
    std::vector<char> buf;
    std::vector<unsigned char> zbuf;
    void flush()
    {
        if (!buf.empty() && fwrite(buf.data(), 1, buf.size(), f) != buf.size()) ok = false;
        buf.clear();
    }
    void raw(const void* p, size_t n)
    {
        const char* c = (const char*)p;
        if (n) buf.insert(buf.end(), c, c + n);
        at += n;
        if (buf.size() >= (size_t)1 << 20) flush();
    }
    template <typename T> void put(T v) { raw(&v, sizeof(T)); }
    void str(const std::string& s) { put<uint32_t>((uint32_t)s.size()); raw(s.data(), s.size()); }   // util/Name.h:57-63
    size_t pos() const { return at; }
    void patch64(size_t where, int64_t v)
    {
        flush();
        if (fseeko(f, (off_t)where, SEEK_SET) != 0 || fwrite(&v, 1, 8, f) != 8 || fseeko(f, 0, SEEK_END) != 0) ok = false;
    }
    // writeData (io/Compression.h:253-264): zipToStream with COMPRESS_ZIP, the raw bytes otherwise
    void data(const void* p, size_t n, uint32_t compression)
    {
        if (!(compression & COMPRESS_ZIP)) { raw(p, n); return; }
        const int64_t head = zip_frame(p, n, zbuf);
        put<int64_t>(head);
        if (head > 0) raw(zbuf.data(), (size_t)head);
        else raw(p, n);
    }
};

// ---- header (io/Archive.cc:939-971), the empty file-level metadata map and the grid count ----
inline void file_header(Out& o, int32_t n_grids)
{
    o.put<int64_t>(0x56444220);            // OPENVDB_MAGIC, version.h:83
    o.put<uint32_t>(224);                  // OPENVDB_FILE_VERSION, version.h:96
    o.put<uint32_t>(4); o.put<uint32_t>(0);  // library 4.0
    o.put<char>(1);                        // seekable: grid offsets follow each descriptor (io::File)
    std::mt19937 ran((unsigned)(std::random_device()() + (unsigned)std::time(nullptr)));
    char u[37];
    const uint32_t a = ran(), b = ran(), c = ran(), d = ran();
    // random (version 4) uuid, textual form of boost::uuids::operator<<
    snprintf(u, sizeof(u), "%08x-%04x-4%03x-%04x-%04x%08x", a, b >> 16, b & 0xfff, 0x8000 | (c >> 18), c & 0xffff, d);
    o.raw(u, 36);
    o.put<uint32_t>(0);                    // file-level metadata: empty map
    o.put<int32_t>(n_grids);
}

// one entry of a metadata map (MetaMap.cc:126-135, Metadata.h:189-218): name, type name, byte count, the value's bytes
struct Meta {
    const char *name, *type;
    std::string value;
};
inline void meta(Out& o, const Meta& m) { o.str(m.name); o.str(m.type); o.str(m.value); }

// the statistics Archive::writeGrid adds to a grid's metadata (Grid.cc:446-457), in std::map order = by name
inline std::vector<Meta> file_stats(uint32_t compression, const int32_t bmin[3], const int32_t bmax[3], int64_t mem_bytes, int64_t voxels)
{
    auto bytes = [](const void* p, size_t n) { return std::string((const char*)p, n); };
    return {{"file_bbox_max", "vec3i", bytes(bmax, 12)},
            {"file_bbox_min", "vec3i", bytes(bmin, 12)},
            {"file_compression", "string", (compression & COMPRESS_ZIP) ? "zip + active values" : "active values"},   // io/Compression.cc:48-58
            {"file_mem_bytes", "int64", bytes(&mem_bytes, 8)},
            {"file_voxel_count", "int64", bytes(&voxels, 8)}};
}

// transform: UniformScaleMap(dx) = scale, voxel size, 1/scale, 1/scale^2, 1/(2 scale) (math/Transform.cc:178-186, math/Maps.h ScaleMap::write)
inline void uniform_scale_map(Out& o, double dx)
{
    o.str("UniformScaleMap");
    const double sc[3] = {dx, dx, dx}, inv[3] = {1 / dx, 1 / dx, 1 / dx}, inv2[3] = {1 / (dx * dx), 1 / (dx * dx), 1 / (dx * dx)},
                 invt[3] = {1 / (2 * dx), 1 / (2 * dx), 1 / (2 * dx)};
    o.raw(sc, 24); o.raw(sc, 24); o.raw(inv, 24); o.raw(inv2, 24); o.raw(invt, 24);
}

// Everything of a grid in front of its root's children: descriptor (io/GridDescriptor.cc:53-73), compression flags, metadata
// (entries in std::map order = by name), transform, the root's head.  Returns the position of the descriptor's three stream
// offsets: the grid position is patched in here, the block position (+8) and the end position (+16) are the caller's.
inline size_t grid_head(Out& o, const std::string& name, uint32_t compression, const std::vector<Meta>& metadata, double voxel_size,
                        float background, uint32_t n_root_children)
{
    o.str(name);
    o.str("Tree_float_5_4_3");
    o.str("");                         // not an instance
    const size_t off = o.pos();
    o.put<int64_t>(0); o.put<int64_t>(0); o.put<int64_t>(0);
    o.patch64(off, (int64_t)o.pos());  // grid position
    o.put<uint32_t>(compression);
    o.put<uint32_t>((uint32_t)metadata.size());
    for (const Meta& m : metadata) meta(o, m);
    uniform_scale_map(o, voxel_size);
    o.put<int32_t>(1);                 // buffer count
    o.put<float>(background);
    o.put<uint32_t>(0);                // root tiles
    o.put<uint32_t>(n_root_children);
    return off;
}

// what follows the child mask of an internal node with no active tile and background tile values: all-off value mask, metadata
// byte 0 (writeCompressedValues: every inactive value == background, 0 active values; child slots are skipped, Compression.h:506)
// and the empty value array through writeData: an int64 0 with ZIP
inline void background_tiles(Out& o, size_t mask_bytes, uint32_t compression)
{
    const std::vector<char> zero(mask_bytes, 0);
    o.raw(zero.data(), mask_bytes);
    o.put<int8_t>(NO_MASK_OR_INACTIVE_VALS);
    o.data(nullptr, 0, compression);
}

// Grid::memUsage() = Tree::memUsage() of a tree with these node counts, as the library reports it in file_mem_bytes
// (Grid.h:778, tree/Tree.h:387, RootNode.h:1463-1472, InternalNode.h:1115-1123, LeafNode.h:1471-1476, LeafBuffer.h:377-387),
// with the x86-64 layouts of OpenVDB 4.0.2 (ABI 3+):
//   LeafNode<float,3>   sizeof 96 (16 B buffer object + 64 B value mask + 12 B origin, padded) + 2048 B of voxels
//   InternalNode<.,4>   4096 unions of 8 B + two 512 B masks + 12 B origin;  InternalNode<.,5>: 32768 x 8 + 2 x 4096 + 12
//   RootNode            sizeof 56 (std::map + background);  Tree: vptr + root + two accessor registries
//                       (tbb::concurrent_hash_map: its size depends on the TBB release — 568 B taken; informational metadata)
inline int64_t tree_mem_bytes(int64_t n_root_children, int64_t n_int1, int64_t n_leaves)
{
    const int64_t leaf = 96 + 2048, int1 = 4096 * 8 + 512 + 512 + 12, int2 = 32768 * 8 + 4096 + 4096 + 12;
    const int64_t root = 56, tree = 8 + 56 + 2 * 568;
    return tree + root + n_root_children * int2 + n_int1 * int1 + n_leaves * leaf;
}

}  // namespace
