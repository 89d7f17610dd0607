// .vdb writer for the step's output FloatGrid — host only, no GPU, no OpenVDB.
//
// Writes what `openvdb::io::File(name).write(grids)` of the reference's OpenVDB 4.0.2 writes for grids created as in
// fluid.cc:1161-1164 (FloatGrid::create(0), linear transform of voxel size 1, fill([lo,hi]^3, 0, active) +
// voxelizeActiveTiles, unnamed) — restated from the library's serialisation code, file format version 224:
//   header            io/Archive.cc:939-971   magic (int64), file version 224, library 4.0, has-offsets flag, 36-char uuid
//   file metadata     MetaMap.cc:117-136      (empty map: count 0)
//   grid count        io/Archive.cc:1167-1173
//   per grid          io/Archive.cc:1243-1328 descriptor (unique name, "Tree_float_5_4_3", instance parent; three stream
//                                             offsets, io/GridDescriptor.cc:53-73), compression flags (:704-723), metadata
//                                             with the file_* statistics (Grid.cc:446-457), transform (math/Transform.cc:
//                                             178-186, math/Maps.h ScaleMap::write), topology, buffers
//   tree              tree/Tree.h:1297-1301,1439-1443  buffer count 1, then the root
//   RootNode          tree/RootNode.h:2257-2288,2407-2412  background, #tiles, #children, children by ascending origin
//   InternalNode      tree/InternalNode.h:2175-2195,3032-3037  child mask, value mask, compressed tile values, children
//   LeafNode          tree/LeafNode.h:1321-1324,1444-1453  value mask (topology); value mask again + compressed values
//   node values       io/Compression.h:462-639  one metadata byte per node; with COMPRESS_ACTIVE_MASK and every inactive
//                                              value equal to the background only the active values follow
//   masks             util/NodeMasks.h:565-568  raw 64-bit words, bit n of word n>>6
//   offsets           tree/LeafNode.h:1049-1055, tree/InternalNode.h:3098-3103  x-major, z fastest
// Compression: COMPRESS_ZIP | COMPRESS_ACTIVE_MASK by default — the library's default without Blosc
// (io/Compression.h:78-81; io/Archive.cc DEFAULT_COMPRESSION_FLAGS) — every value buffer goes through zipToStream
// (io/Compression.cc:70-100: compress2 at Z_DEFAULT_COMPRESSION, an int64 byte count in front, negative and followed by the
// raw bytes when zipping did not shrink the buffer); FLUID_VDB_ACTIVE_MASK alone is kept for readers without zlib.
// Which grids go into which file (fluid.cc:1366-1373,1450-1451,1503-1508): `grids2` is declared INSIDE the step loop, so
// simulation/mygrids<i>.vdb holds exactly the grid of step i; `grids` is declared outside it and grows by one grid per
// step, so the final mygrids.vdb holds every step's grid (500 of them) — written here as a stream, one grid appended per
// step (fluid_vdb_open / _append / _close), names get the "\x1e<k>" suffixes of io/Archive.cc:1196-1206.
// Parity status: UNPINNED against the real library (no OpenVDB here to read the files back, no sample .vdb in the
// reference tree); tests/test_vdb.py re-reads the files with an independent restatement of the READ side.
#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <map>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "fluid_hip.h"

namespace {

// buffered stream to the file (a 512^3 grid is 0.6 GB: nothing is held in memory); offsets are patched by seeking back
struct Out {
    FILE* f = nullptr;
    size_t at = 0;
    bool ok = true;
    std::vector<char> buf;
    void flush()
    {
        if (!buf.empty() && fwrite(buf.data(), 1, buf.size(), f) != buf.size()) ok = false;
        buf.clear();
    }
    void raw(const void* p, size_t n)
    {
        const char* c = (const char*)p;
        buf.insert(buf.end(), c, c + n);
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
    std::vector<unsigned char> zbuf;
    void data(const void* p, size_t n, uint32_t compression)
    {
        if (!(compression & 0x1)) { raw(p, n); return; }
        uLongf zn = compressBound((uLong)n);
        zbuf.resize(zn);
        const int st = compress2(zbuf.data(), &zn, (const Bytef*)p, (uLong)n, Z_DEFAULT_COMPRESSION);
        if (st == Z_OK && zn < n) {
            put<int64_t>((int64_t)zn);
            raw(zbuf.data(), zn);
        } else {
            put<int64_t>(-(int64_t)n);
            raw(p, n);
        }
    }
};

inline int floor_to(int v, int m) { return v & ~(m - 1); }  // origin of the node of size m (power of two) that holds v

constexpr int LEAF = 8, INT1 = 128, INT2 = 4096;             // Tree_float_5_4_3: 8^3 leaves, 16^3 of them, 32^3 of those
constexpr uint32_t COMPRESS_ZIP = 0x1, COMPRESS_ACTIVE_MASK = 0x2;   // io/Compression.h:79-80
constexpr int8_t NO_MASK_OR_INACTIVE_VALS = 0;               // io/Compression.h:94

struct Dense {
    int n, lo, hi;
    const float* v;
    bool inside(int x, int y, int z) const { return x >= lo && x <= hi && y >= lo && y <= hi && z >= lo && z <= hi; }
    float at(int x, int y, int z) const { return v[((size_t)(x - lo) * n + (y - lo)) * n + (z - lo)]; }
    bool overlaps(int ox, int oy, int oz, int dim) const
    {
        return ox + dim - 1 >= lo && ox <= hi && oy + dim - 1 >= lo && oy <= hi && oz + dim - 1 >= lo && oz <= hi;
    }
};

// value mask of the leaf at (ox,oy,oz): voxels inside the box are active (fill(..., active=true), fluid.cc:1163)
void leaf_mask(const Dense& g, int ox, int oy, int oz, uint64_t m[8])
{
    for (int w = 0; w < 8; ++w) m[w] = 0;
    for (int x = 0; x < 8; ++x)
        for (int y = 0; y < 8; ++y)
            for (int z = 0; z < 8; ++z)
                if (g.inside(ox + x, oy + y, oz + z)) {
                    const int n = (x << 6) + (y << 3) + z;
                    m[n >> 6] |= 1ull << (n & 63);
                }
}

// an internal node with no active tiles and background tile values: all-off value mask, metadata byte 0, no values
void internal_values(Out& o, size_t mask_bytes, uint32_t compression)
{
    std::vector<char> zero(mask_bytes, 0);
    o.raw(zero.data(), mask_bytes);          // mValueMask
    o.put<int8_t>(NO_MASK_OR_INACTIVE_VALS);   // writeCompressedValues: every inactive value == background, 0 active values
    o.data(nullptr, 0, compression);           // ... and the (empty) value array through writeData: an int64 0 with ZIP
}

// One leaf of the buffers pass: mask, active values, and (ZIP) the zipToStream framing of the values, prepared off the output
// stream so that the leaves of a 128^3 node can be compressed on several host threads (zlib at the library's default level costs
// ~20 us per leaf: 80 ms for a 121^3 grid on one thread, written twice per step by the driver); the bytes are those of the
// serial path, in the same order.
struct LeafJob {
    int lx, ly, lz;
    uint64_t vm[8];
    int na;
    float act[512];
    int64_t head;                       // zip: the int64 in front (compressed size, or -raw size)
    std::vector<unsigned char> z;       // zip: the compressed bytes (empty: the raw values follow)
};
// zipToStream's framing of na floats: the int64 in front (compressed size, or -raw size when zipping did not shrink them: the
// raw bytes then follow and z is left empty)
int64_t zip_values(const float* act, int na, std::vector<unsigned char>& z)
{
    const size_t n = (size_t)na * sizeof(float);
    uLongf zn = compressBound((uLong)n);
    z.resize(zn);
    const int st = compress2(z.data(), &zn, (const Bytef*)act, (uLong)n, Z_DEFAULT_COMPRESSION);
    if (st == Z_OK && zn < n) { z.resize(zn); return (int64_t)zn; }
    z.clear();
    return -(int64_t)n;
}
void prepare_leaf(const Dense& g, LeafJob& j, uint32_t compression)
{
    leaf_mask(g, j.lx, j.ly, j.lz, j.vm);
    j.na = 0;
    for (int x = 0; x < 8; ++x)
        for (int y = 0; y < 8; ++y)
            for (int z = 0; z < 8; ++z)
                if (g.inside(j.lx + x, j.ly + y, j.lz + z)) j.act[j.na++] = g.at(j.lx + x, j.ly + y, j.lz + z);
    j.z.clear();
    j.head = 0;
    if (compression & COMPRESS_ZIP) j.head = zip_values(j.act, j.na, j.z);
}
void flush_leaves(Out& o, const Dense& g, std::vector<LeafJob>& jobs, uint32_t compression)
{
    const size_t n = jobs.size();
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : (nt > 16 ? 16 : nt);
    if (n < 64 || !(compression & COMPRESS_ZIP)) nt = 1;
    if (nt == 1) {
        for (auto& j : jobs) prepare_leaf(g, j, compression);
    } else {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; ++t)
            th.emplace_back([&, t] { for (size_t i = t; i < n; i += nt) prepare_leaf(g, jobs[i], compression); });
        for (auto& x : th) x.join();
    }
    for (auto& j : jobs) {
        o.raw(j.vm, sizeof(j.vm));
        o.put<int8_t>(NO_MASK_OR_INACTIVE_VALS);  // inactive voxels hold the background
        if (compression & COMPRESS_ZIP) {
            o.put<int64_t>(j.head);
            if (j.head > 0) o.raw(j.z.data(), j.z.size());
            else o.raw(j.act, (size_t)j.na * sizeof(float));
        } else {
            o.raw(j.act, (size_t)j.na * sizeof(float));
        }
    }
    jobs.clear();
}

void write_tree(Out& o, const Dense& g, bool buffers, uint32_t compression)
{
    std::vector<LeafJob> jobs;
    // root children in ascending (x,y,z) origin order (std::map<Coord>, math/Coord.h:180-185)
    for (int rx = floor_to(g.lo, INT2); rx <= g.hi; rx += INT2)
        for (int ry = floor_to(g.lo, INT2); ry <= g.hi; ry += INT2)
            for (int rz = floor_to(g.lo, INT2); rz <= g.hi; rz += INT2) {
                if (!buffers) {
                    const int32_t org[3] = {rx, ry, rz};
                    o.raw(org, sizeof(org));
                    std::vector<uint64_t> cm(32 * 32 * 32 / 64, 0);  // child mask of the 4096^3 node: 32^3 slots of 128^3
                    for (int a = 0; a < 32; ++a)
                        for (int b = 0; b < 32; ++b)
                            for (int c = 0; c < 32; ++c)
                                if (g.overlaps(rx + a * INT1, ry + b * INT1, rz + c * INT1, INT1)) {
                                    const int n = (a << 10) + (b << 5) + c;
                                    cm[n >> 6] |= 1ull << (n & 63);
                                }
                    o.raw(cm.data(), cm.size() * 8);
                    internal_values(o, cm.size() * 8, compression);
                }
                for (int a = 0; a < 32; ++a)
                    for (int b = 0; b < 32; ++b)
                        for (int c = 0; c < 32; ++c) {
                            const int ix = rx + a * INT1, iy = ry + b * INT1, iz = rz + c * INT1;
                            if (!g.overlaps(ix, iy, iz, INT1)) continue;
                            if (!buffers) {
                                uint64_t cm[64] = {};  // 16^3 slots of 8^3
                                for (int p = 0; p < 16; ++p)
                                    for (int q = 0; q < 16; ++q)
                                        for (int r = 0; r < 16; ++r)
                                            if (g.overlaps(ix + p * LEAF, iy + q * LEAF, iz + r * LEAF, LEAF)) {
                                                const int n = (p << 8) + (q << 4) + r;
                                                cm[n >> 6] |= 1ull << (n & 63);
                                            }
                                o.raw(cm, sizeof(cm));
                                internal_values(o, sizeof(cm), compression);
                            }
                            for (int p = 0; p < 16; ++p)
                                for (int q = 0; q < 16; ++q)
                                    for (int r = 0; r < 16; ++r) {
                                        const int lx = ix + p * LEAF, ly = iy + q * LEAF, lz = iz + r * LEAF;
                                        if (!g.overlaps(lx, ly, lz, LEAF)) continue;
                                        if (buffers) {   // (the leaves of this 128^3 node are written below, together)
                                            jobs.emplace_back();
                                            jobs.back().lx = lx; jobs.back().ly = ly; jobs.back().lz = lz;
                                            continue;
                                        }
                                        uint64_t vm[8];
                                        leaf_mask(g, lx, ly, lz, vm);
                                        o.raw(vm, sizeof(vm));
                                    }
                            if (buffers) flush_leaves(o, g, jobs, compression);
                        }
            }
}

template <typename T> void meta(Out& o, const char* name, const char* type, const T* v, uint32_t bytes)
{
    o.str(name); o.str(type); o.put<uint32_t>(bytes); o.raw(v, bytes);   // MetaMap.cc:126-135, Metadata.h:189-218
}

// Grid::memUsage() = Tree::memUsage() of the tree this file describes, as the library reports it in file_mem_bytes
// (Grid.h:778, tree/Tree.h:387, RootNode.h:1463-1472, InternalNode.h:1115-1123, LeafNode.h:1471-1476, LeafBuffer.h:377-387),
// with the x86-64 layouts of OpenVDB 4.0.2 (ABI 3+):
//   LeafNode<float,3>   sizeof 96 (16 B buffer object + 64 B value mask + 12 B origin, padded) + 2048 B of voxels
//   InternalNode<.,4>   4096 unions of 8 B + two 512 B masks + 12 B origin;  InternalNode<.,5>: 32768 x 8 + 2 x 4096 + 12
//   RootNode            sizeof 56 (std::map + background);  Tree: vptr + root + two accessor registries
//                       (tbb::concurrent_hash_map: its size depends on the TBB release — 568 B taken; informational metadata)
int64_t tree_mem_bytes(int lo, int hi)
{
    auto count = [&](int dim) { long c = 0; for (int x = floor_to(lo, dim); x <= hi; x += dim) ++c; return c * c * c; };
    const int64_t leaves = count(LEAF), n1 = count(INT1), n2 = count(INT2);
    const int64_t leaf = 96 + 2048, int1 = 4096 * 8 + 512 + 512 + 12, int2 = 32768 * 8 + 4096 + 4096 + 12;
    const int64_t root = 56, tree = 8 + 56 + 2 * 568;
    return tree + root + n2 * int2 + n1 * int1 + leaves * leaf;
}

struct Writer {
    Out o;
    int n = 0, n_grids = 0, written = 0;
    uint32_t compression = 0;
    std::map<int, std::vector<unsigned char>> zero_values;   // leaf path: the value bytes of a leaf of na zeros, by na
};

int writer_open(Writer& w, const char* path, int32_t n, int32_t n_grids, int32_t compression)
{
    w.n = n; w.n_grids = n_grids; w.written = 0;
    w.compression = (uint32_t)compression;
    Out& o = w.o;
    o.f = fopen(path, "wb");
    if (!o.f) return FLUID_ERR_ARG;
    // ---- header (io/Archive.cc:939-971) ----
    o.put<int64_t>(0x56444220);            // OPENVDB_MAGIC, version.h:83
    o.put<uint32_t>(224);                  // OPENVDB_FILE_VERSION, version.h:96
    o.put<uint32_t>(4); o.put<uint32_t>(0);  // library 4.0
    o.put<char>(1);                        // seekable: grid offsets follow each descriptor (io::File)
    {
        std::mt19937 ran((unsigned)(std::random_device()() + (unsigned)std::time(nullptr)));
        char u[37];
        const uint32_t a = ran(), b = ran(), c = ran(), d = ran();
        // random (version 4) uuid, textual form of boost::uuids::operator<<
        snprintf(u, sizeof(u), "%08x-%04x-4%03x-%04x-%04x%08x", a, b >> 16, b & 0xfff, 0x8000 | (c >> 18), c & 0xffff, d);
        o.raw(u, 36);
    }
    o.put<uint32_t>(0);                    // file-level metadata: empty map
    o.put<int32_t>(n_grids);
    return FLUID_OK;
}

// everything of a grid in front of its tree: descriptor, compression flags, metadata, transform, the root's head.
// Returns the position of the descriptor's three stream offsets (the grid position is already patched in).
size_t grid_head(Writer& w)
{
    Out& o = w.o;
    const int n = w.n, k = w.written;
    const int lo = -(n / 2), hi = lo + n - 1;
    // ---- descriptor (io/GridDescriptor.cc:53-73); unnamed grids become "\x1e<k>" (io/Archive.cc:1196-1206) ----
    o.str(std::string("\x1e") + std::to_string(k));
    o.str("Tree_float_5_4_3");
    o.str("");                         // not an instance
    const size_t off = o.pos();
    o.put<int64_t>(0); o.put<int64_t>(0); o.put<int64_t>(0);
    o.patch64(off, (int64_t)o.pos());  // grid position
    o.put<uint32_t>(w.compression);
    // ---- grid metadata: the statistics Archive::writeGrid adds (std::map order = by name) ----
    const int32_t bmin[3] = {lo, lo, lo}, bmax[3] = {hi, hi, hi};
    const int64_t voxels = (int64_t)n * n * n, mem = tree_mem_bytes(lo, hi);
    const std::string comp = (w.compression & COMPRESS_ZIP) ? "zip + active values" : "active values";  // io/Compression.cc:48-58
    o.put<uint32_t>(5);
    meta(o, "file_bbox_max", "vec3i", bmax, 12);
    meta(o, "file_bbox_min", "vec3i", bmin, 12);
    meta(o, "file_compression", "string", comp.data(), (uint32_t)comp.size());
    meta(o, "file_mem_bytes", "int64", &mem, 8);
    meta(o, "file_voxel_count", "int64", &voxels, 8);
    // ---- transform: UniformScaleMap(1.0) = scale, voxel size, 1/scale, 1/scale^2, 1/(2 scale) ----
    o.str("UniformScaleMap");
    const double one[3] = {1, 1, 1}, half[3] = {0.5, 0.5, 0.5};
    o.raw(one, 24); o.raw(one, 24); o.raw(one, 24); o.raw(one, 24); o.raw(half, 24);
    // ---- topology ----
    o.put<int32_t>(1);                 // buffer count
    o.put<float>(0.0f);                // background
    o.put<uint32_t>(0);                // root tiles
    uint32_t nroot = 0;
    for (int x = floor_to(lo, INT2); x <= hi; x += INT2) ++nroot;
    o.put<uint32_t>(nroot * nroot * nroot);
    return off;
}

int writer_append(Writer& w, const float* grid)
{
    if (w.written >= w.n_grids) return FLUID_ERR_STATE;
    Out& o = w.o;
    const int n = w.n;
    const int lo = -(n / 2), hi = lo + n - 1;
    const Dense g{n, lo, hi, grid};
    const size_t off = grid_head(w);
    write_tree(o, g, false, w.compression);
    o.patch64(off + 8, (int64_t)o.pos());   // block position
    write_tree(o, g, true, w.compression);
    o.patch64(off + 16, (int64_t)o.pos());  // end position
    w.written++;
    return o.ok ? FLUID_OK : FLUID_ERR_ARG;
}

int writer_close(Writer& w)
{
    w.o.flush();
    const int rc = w.o.f ? fclose(w.o.f) : 0;
    w.o.f = nullptr;
    return (w.o.ok && rc == 0 && w.written == w.n_grids) ? FLUID_OK : FLUID_ERR_ARG;
}

// ---- the same grid from the list of its non-zero leaves (fluid_vdb_append_leaves) ---------------------------------------------
// The file is the dense path's, byte for byte: every leaf of [lo,hi]^3 is written with its full value mask.  What differs is the
// work: a leaf the list does not name holds zeros only, so its value bytes are a constant of its active-voxel count; masks come
// from the leaf's per-axis in-grid ranges (a leaf is the first, an inner or the last of its axis: 4 classes per axis, 64 masks);
// the listed leaves are gathered and zipped once for all writers of the call.
struct LeafGeom {
    int n, lo, hi, L0, nl;
    int a0[4], a1[4];              // in-grid voxel range of a leaf by axis class: bit 0 = first leaf of the axis, bit 1 = last
    uint64_t mask[64][8];          // value mask by (cx * 4 + cy) * 4 + cz
    int na[64];
    explicit LeafGeom(int n_) : n(n_), lo(-(n_ / 2)), hi(lo + n_ - 1), L0(floor_to(lo, LEAF)), nl((floor_to(hi, LEAF) - L0) / LEAF + 1)
    {
        for (int c = 0; c < 4; ++c) {
            a0[c] = (c & 1) ? lo - L0 : 0;
            a1[c] = (c & 2) ? hi - floor_to(hi, LEAF) : LEAF - 1;
        }
        for (int cx = 0; cx < 4; ++cx)
            for (int cy = 0; cy < 4; ++cy)
                for (int cz = 0; cz < 4; ++cz) {
                    const int c = (cx * 4 + cy) * 4 + cz;
                    na[c] = 0;
                    for (int x = 0; x < 8; ++x) mask[c][x] = 0;
                    if (a1[cx] < a0[cx] || a1[cy] < a0[cy] || a1[cz] < a0[cz]) continue;   // "first and last" of an axis with several leaves: no such leaf
                    const uint64_t zb = ((1ull << (a1[cz] - a0[cz] + 1)) - 1) << a0[cz];   // one (x, y) row: bits z
                    uint64_t word = 0;                                                     // one x: 8 rows
                    for (int y = a0[cy]; y <= a1[cy]; ++y) word |= zb << (8 * y);
                    for (int x = 0; x < 8; ++x) mask[c][x] = (x >= a0[cx] && x <= a1[cx]) ? word : 0;
                    na[c] = (a1[cx] - a0[cx] + 1) * (a1[cy] - a0[cy] + 1) * (a1[cz] - a0[cz] + 1);
                }
    }
    int axis_class(int i) const { return (i == 0 ? 1 : 0) | (i == nl - 1 ? 2 : 0); }
    int leaf_class(int i, int j, int k) const { return (axis_class(i) * 4 + axis_class(j)) * 4 + axis_class(k); }
};

// FLUID_OK, or FLUID_ERR_ARG: an origin off the 8-grid, outside the leaves of [lo,hi]^3, or not strictly ascending in (x, y, z)
int check_leaf_list(const fluid_leaf_grid_t* g)
{
    if (!g || g->n < 1 || g->n > 4096 || g->n_leaves < 0) return FLUID_ERR_ARG;
    if (g->n_leaves > 0 && (!g->origin || !g->values)) return FLUID_ERR_ARG;
    const int lo = -(g->n / 2), hi = lo + g->n - 1, L0 = floor_to(lo, LEAF), L1 = floor_to(hi, LEAF);
    for (int i = 0; i < g->n_leaves; ++i) {
        const int32_t* o = g->origin + 3 * (size_t)i;
        for (int a = 0; a < 3; ++a)
            if ((o[a] & (LEAF - 1)) != 0 || o[a] < L0 || o[a] > L1) return FLUID_ERR_ARG;
        if (i > 0) {
            const int32_t* p = o - 3;
            const bool after = o[0] != p[0] ? o[0] > p[0] : o[1] != p[1] ? o[1] > p[1] : o[2] > p[2];
            if (!after) return FLUID_ERR_ARG;
        }
    }
    return FLUID_OK;
}

// the bytes that follow a leaf's metadata byte in the buffers pass, for its na active values
void value_bytes(const float* act, int na, uint32_t compression, std::vector<unsigned char>& out, std::vector<unsigned char>& z)
{
    const unsigned char* raw = (const unsigned char*)act;
    const size_t n = (size_t)na * sizeof(float);
    if (!(compression & COMPRESS_ZIP)) { out.insert(out.end(), raw, raw + n); return; }
    const int64_t head = zip_values(act, na, z);
    out.insert(out.end(), (const unsigned char*)&head, (const unsigned char*)&head + 8);
    if (head > 0) out.insert(out.end(), z.begin(), z.end());
    else out.insert(out.end(), raw, raw + n);
}

struct Span { const unsigned char* p; size_t n; };

// every writer of the call receives the same bytes
struct Fan {
    Writer* const* w;
    int n;
    void raw(const void* p, size_t len) const { for (int i = 0; i < n; ++i) w[i]->o.raw(p, len); }
};

void write_tree_leaves(const Fan& f, const LeafGeom& G, bool buffers, uint32_t compression, const std::vector<int>& table,
                       const std::vector<Span>& listed, const Span zero[64])
{
    const Dense g{G.n, G.lo, G.hi, nullptr};   // the box tests of write_tree; no value is read through it
    const int8_t meta_byte = NO_MASK_OR_INACTIVE_VALS;
    std::vector<unsigned char> chunk;
    auto add = [&](const void* p, size_t len) { chunk.insert(chunk.end(), (const unsigned char*)p, (const unsigned char*)p + len); };
    for (int rx = floor_to(g.lo, INT2); rx <= g.hi; rx += INT2)
        for (int ry = floor_to(g.lo, INT2); ry <= g.hi; ry += INT2)
            for (int rz = floor_to(g.lo, INT2); rz <= g.hi; rz += INT2) {
                if (!buffers) {
                    const int32_t org[3] = {rx, ry, rz};
                    f.raw(org, sizeof(org));
                    std::vector<uint64_t> cm(32 * 32 * 32 / 64, 0);
                    for (int a = 0; a < 32; ++a)
                        for (int b = 0; b < 32; ++b)
                            for (int c = 0; c < 32; ++c)
                                if (g.overlaps(rx + a * INT1, ry + b * INT1, rz + c * INT1, INT1)) {
                                    const int n = (a << 10) + (b << 5) + c;
                                    cm[n >> 6] |= 1ull << (n & 63);
                                }
                    f.raw(cm.data(), cm.size() * 8);
                    for (int i = 0; i < f.n; ++i) internal_values(f.w[i]->o, cm.size() * 8, compression);
                }
                for (int a = 0; a < 32; ++a)
                    for (int b = 0; b < 32; ++b)
                        for (int c = 0; c < 32; ++c) {
                            const int ix = rx + a * INT1, iy = ry + b * INT1, iz = rz + c * INT1;
                            if (!g.overlaps(ix, iy, iz, INT1)) continue;
                            if (!buffers) {
                                uint64_t cm[64] = {};
                                for (int p = 0; p < 16; ++p)
                                    for (int q = 0; q < 16; ++q)
                                        for (int r = 0; r < 16; ++r)
                                            if (g.overlaps(ix + p * LEAF, iy + q * LEAF, iz + r * LEAF, LEAF)) {
                                                const int n = (p << 8) + (q << 4) + r;
                                                cm[n >> 6] |= 1ull << (n & 63);
                                            }
                                f.raw(cm, sizeof(cm));
                                for (int i = 0; i < f.n; ++i) internal_values(f.w[i]->o, sizeof(cm), compression);
                            }
                            for (int p = 0; p < 16; ++p)
                                for (int q = 0; q < 16; ++q)
                                    for (int r = 0; r < 16; ++r) {
                                        const int lx = ix + p * LEAF, ly = iy + q * LEAF, lz = iz + r * LEAF;
                                        if (!g.overlaps(lx, ly, lz, LEAF)) continue;
                                        const int i = (lx - G.L0) / LEAF, j = (ly - G.L0) / LEAF, k = (lz - G.L0) / LEAF;
                                        const int cls = G.leaf_class(i, j, k);
                                        add(G.mask[cls], sizeof(G.mask[cls]));
                                        if (!buffers) continue;
                                        add(&meta_byte, 1);
                                        const int t = table[((size_t)i * G.nl + j) * G.nl + k];
                                        const Span& s = t >= 0 ? listed[(size_t)t] : zero[cls];
                                        add(s.p, s.n);
                                    }
                            f.raw(chunk.data(), chunk.size());   // the leaves of this 128^3 node, to every writer at once
                            chunk.clear();
                        }
            }
}

int append_leaves(Writer* const* ws, int nw, const fluid_leaf_grid_t* g)
{
    const uint32_t compression = ws[0]->compression;
    for (int i = 0; i < nw; ++i)
        if (ws[i]->n != g->n || ws[i]->compression != compression) return FLUID_ERR_ARG;
    int rc = check_leaf_list(g);
    if (rc) return rc;
    for (int i = 0; i < nw; ++i)
        if (ws[i]->written >= ws[i]->n_grids) return FLUID_ERR_STATE;
    const LeafGeom G(g->n);
    const size_t nlist = (size_t)g->n_leaves;
    // table over the grid's leaves: the tree walk (root -> 128^3 nodes -> leaves) is not the list's order for N > 128
    std::vector<int> table((size_t)G.nl * G.nl * G.nl, -1);
    std::vector<int> cls(nlist);
    for (size_t t = 0; t < nlist; ++t) {
        const int32_t* o = g->origin + 3 * t;
        const int i = (o[0] - G.L0) / LEAF, j = (o[1] - G.L0) / LEAF, k = (o[2] - G.L0) / LEAF;
        table[((size_t)i * G.nl + j) * G.nl + k] = (int)t;
        cls[t] = G.leaf_class(i, j, k);
    }
    // the listed leaves' value bytes, once for every writer: contiguous shares of the list on at most 16 threads
    const bool zip = (compression & COMPRESS_ZIP) != 0;
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : (nt > 16 ? 16 : nt);
    if (nlist < 64 || !zip) nt = 1;
    std::vector<std::vector<unsigned char>> arena(nt);
    std::vector<size_t> at(nlist), len(nlist);
    auto share = [&](unsigned t) {
        std::vector<unsigned char> z;
        float act[512];
        for (size_t l = nlist * t / nt; l < nlist * (t + 1) / nt; ++l) {
            const int c = cls[l], cx = c >> 4, cy = (c >> 2) & 3, cz = c & 3;
            const float* v = g->values + 512 * l;
            at[l] = arena[t].size();
            if (!zip && G.na[c] == 512) { len[l] = 0; continue; }   // a whole leaf, stored raw: written straight from the list
            int na = 0;
            for (int x = G.a0[cx]; x <= G.a1[cx]; ++x)
                for (int y = G.a0[cy]; y <= G.a1[cy]; ++y)
                    for (int zz = G.a0[cz]; zz <= G.a1[cz]; ++zz) act[na++] = v[(x * 8 + y) * 8 + zz];
            value_bytes(act, na, compression, arena[t], z);
            len[l] = arena[t].size() - at[l];
        }
    };
    if (nt == 1) {
        share(0);
    } else {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; ++t) th.emplace_back(share, t);
        for (auto& x : th) x.join();
    }
    std::vector<Span> listed(nlist);
    for (unsigned t = 0; t < nt; ++t)
        for (size_t l = nlist * t / nt; l < nlist * (t + 1) / nt; ++l) {
            if (len[l] == 0) listed[l] = Span{(const unsigned char*)(g->values + 512 * l), 2048};
            else listed[l] = Span{arena[t].data() + at[l], len[l]};
        }
    // unlisted leaves: the value bytes of na zeros, from whichever writer of the call has them already
    Span zero[64];
    {
        std::vector<unsigned char> z;
        const float zeros[512] = {};
        for (int c = 0; c < 64; ++c) {
            const int na = G.na[c];
            const std::vector<unsigned char>* have = nullptr;
            for (int i = 0; i < nw && !have; ++i) {
                auto it = ws[i]->zero_values.find(na);
                if (it != ws[i]->zero_values.end()) have = &it->second;
            }
            std::vector<unsigned char> made;
            if (!have) value_bytes(zeros, na, compression, made, z);
            for (int i = 0; i < nw; ++i)
                if (!ws[i]->zero_values.count(na)) ws[i]->zero_values[na] = have ? *have : made;
            const std::vector<unsigned char>& b = ws[0]->zero_values[na];
            zero[c] = Span{b.data(), b.size()};
        }
    }
    const Fan f{ws, nw};
    std::vector<size_t> off((size_t)nw);
    for (int i = 0; i < nw; ++i) off[(size_t)i] = grid_head(*ws[i]);
    write_tree_leaves(f, G, false, compression, table, listed, zero);
    for (int i = 0; i < nw; ++i) ws[i]->o.patch64(off[(size_t)i] + 8, (int64_t)ws[i]->o.pos());    // block position
    write_tree_leaves(f, G, true, compression, table, listed, zero);
    bool ok = true;
    for (int i = 0; i < nw; ++i) {
        ws[i]->o.patch64(off[(size_t)i] + 16, (int64_t)ws[i]->o.pos());   // end position
        ws[i]->written++;
        ok = ok && ws[i]->o.ok;
    }
    return ok ? FLUID_OK : FLUID_ERR_ARG;
}

}  // namespace

struct fluid_vdb_writer {
    Writer w;
};

extern "C" {

int fluid_vdb_open(const char* path, int32_t n, int32_t n_grids, int32_t compression, fluid_vdb_writer_t** out)
{
    if (!path || n < 1 || n > 4096 || n_grids < 1 || !out) return FLUID_ERR_ARG;
    if (compression != FLUID_VDB_ACTIVE_MASK && compression != FLUID_VDB_ZIP_ACTIVE_MASK) return FLUID_ERR_ARG;
    fluid_vdb_writer* h = new fluid_vdb_writer();
    const int rc = writer_open(h->w, path, n, n_grids, compression);
    if (rc) { delete h; return rc; }
    *out = h;
    return FLUID_OK;
}

int fluid_vdb_append(fluid_vdb_writer_t* h, const float* grid)
{
    if (!h || !grid) return FLUID_ERR_ARG;
    return writer_append(h->w, grid);
}

int fluid_vdb_close(fluid_vdb_writer_t* h)
{
    if (!h) return FLUID_OK;
    const int rc = writer_close(h->w);
    delete h;
    return rc;
}

int fluid_write_vdb_ex(const char* path, int32_t n, int32_t n_grids, const float* const* grids, int32_t compression)
{
    if (!grids) return FLUID_ERR_ARG;
    for (int k = 0; k < n_grids; ++k)
        if (!grids[k]) return FLUID_ERR_ARG;
    fluid_vdb_writer_t* h = nullptr;
    int rc = fluid_vdb_open(path, n, n_grids, compression, &h);
    if (rc) return rc;
    for (int k = 0; k < n_grids && !rc; ++k) rc = fluid_vdb_append(h, grids[k]);
    const int rc2 = fluid_vdb_close(h);
    return rc ? rc : rc2;
}

int fluid_write_vdb(const char* path, int32_t n, int32_t n_grids, const float* const* grids)
{
    return fluid_write_vdb_ex(path, n, n_grids, grids, FLUID_VDB_ZIP_ACTIVE_MASK);
}

int fluid_leaves_to_dense(const fluid_leaf_grid_t* g, float* dense)
{
    if (!dense) return FLUID_ERR_ARG;
    const int rc = check_leaf_list(g);
    if (rc) return rc;
    const int n = g->n, lo = -(n / 2);
    memset(dense, 0, (size_t)n * n * n * sizeof(float));
    for (int l = 0; l < g->n_leaves; ++l) {
        const int32_t* o = g->origin + 3 * (size_t)l;
        const float* v = g->values + 512 * (size_t)l;
        for (int x = 0; x < 8; ++x)
            for (int y = 0; y < 8; ++y)
                for (int z = 0; z < 8; ++z) {
                    const int ax = o[0] + x - lo, ay = o[1] + y - lo, az = o[2] + z - lo;
                    if (ax < 0 || ax >= n || ay < 0 || ay >= n || az < 0 || az >= n) continue;
                    dense[((size_t)ax * n + ay) * n + az] = v[(x * 8 + y) * 8 + z];
                }
    }
    return FLUID_OK;
}

// One k-way merge over the parts' (already ascending) lists, run twice: the first pass counts and checks and writes nothing, the
// second writes.  A leaf listed by one part is copied; one listed by several is OR-ed as bit patterns — exact, because a voxel is
// owned by one part and +0 in the others, which the first pass verifies.
int64_t fluid_leaf_grids_merge(const fluid_leaf_grid_t* parts, int32_t n_parts, int64_t cap_leaves, int32_t* origin, float* values)
{
    if (!parts || n_parts < 1 || (origin == nullptr) != (values == nullptr)) return -FLUID_ERR_ARG;
    for (int p = 0; p < n_parts; ++p)
        if (check_leaf_list(&parts[p]) != FLUID_OK || parts[p].n != parts[0].n) return -FLUID_ERR_ARG;
    auto before = [](const int32_t* a, const int32_t* b) { return a[0] != b[0] ? a[0] < b[0] : a[1] != b[1] ? a[1] < b[1] : a[2] < b[2]; };
    std::vector<int32_t> cur((size_t)n_parts);
    int64_t count = 0;
    for (int pass = 0; pass < (origin ? 2 : 1); ++pass) {
        if (pass == 1 && count > cap_leaves) return -FLUID_ERR_ARG;
        std::fill(cur.begin(), cur.end(), 0);
        count = 0;
        for (;;) {
            const int32_t* o = nullptr;   // the smallest origin at the parts' cursors
            for (int p = 0; p < n_parts; ++p) {
                if (cur[p] >= parts[p].n_leaves) continue;
                const int32_t* c = parts[p].origin + 3 * (size_t)cur[p];
                if (!o || before(c, o)) o = c;
            }
            if (!o) break;
            const int32_t o3[3] = {o[0], o[1], o[2]};
            uint32_t acc[512];
            int n_in = 0;
            for (int p = 0; p < n_parts; ++p) {
                if (cur[p] >= parts[p].n_leaves) continue;
                const int32_t* c = parts[p].origin + 3 * (size_t)cur[p];
                if (c[0] != o3[0] || c[1] != o3[1] || c[2] != o3[2]) continue;
                const float* v = parts[p].values + 512 * (size_t)cur[p];
                cur[p]++;
                if (n_in++ == 0) { memcpy(acc, v, sizeof acc); continue; }
                for (int i = 0; i < 512; ++i) {
                    uint32_t b;
                    memcpy(&b, v + i, sizeof b);
                    if (pass == 0 && b && acc[i]) return -FLUID_ERR_ARG;   // two parts claim the voxel
                    acc[i] |= b;
                }
            }
            if (pass == 1) {
                memcpy(origin + 3 * (size_t)count, o3, sizeof o3);
                memcpy(values + 512 * (size_t)count, acc, sizeof acc);
            }
            count++;
        }
    }
    return count;
}

int fluid_vdb_append_leaves(fluid_vdb_writer_t* const* writers, int32_t n_writers, const fluid_leaf_grid_t* g)
{
    if (!writers || n_writers < 1 || n_writers > 64 || !g) return FLUID_ERR_ARG;
    Writer* ws[64];
    for (int i = 0; i < n_writers; ++i) {
        if (!writers[i]) return FLUID_ERR_ARG;
        for (int j = 0; j < i; ++j)
            if (writers[j] == writers[i]) return FLUID_ERR_ARG;
        ws[i] = &writers[i]->w;
    }
    return append_leaves(ws, n_writers, g);
}

int fluid_write_vdb_leaves(const char* path, const fluid_leaf_grid_t* g, int32_t compression)
{
    if (!g) return FLUID_ERR_ARG;
    int rc = check_leaf_list(g);   // before the file is created
    if (rc) return rc;
    fluid_vdb_writer_t* h = nullptr;
    rc = fluid_vdb_open(path, g->n, 1, compression, &h);
    if (rc) return rc;
    rc = fluid_vdb_append_leaves(&h, 1, g);
    const int rc2 = fluid_vdb_close(h);
    return rc ? rc : rc2;
}

}  // extern "C"
