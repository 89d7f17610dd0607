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
// What this file holds is the tree with every leaf of [lo,hi]^3 present and background 0, from a dense array or from the list of
// its non-zero leaves, and the merge of such lists.  The stream, the zip framing, the header and everything of a grid in front of
// its tree are vdb_format.h's, shared with vdb_sdf_writer.cpp; the list rules, the dense scatter and the merge's walk are
// leaf_list.h's.
// Parity status: UNPINNED against the real library (no OpenVDB here to read the files back, no sample .vdb in the
// reference tree); tests/test_vdb.py re-reads the files with an independent restatement of the READ side, and
// tests/test_vdb_bytes.py holds digests of the bytes.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "vdb_format.h"

namespace {

// The leaves of the box [lo,hi]^3, all of them in the tree with their in-box voxels active (fill(..., active=true), fluid.cc:1163).
// Masks come from a leaf's per-axis in-grid ranges (a leaf is the first, an inner or the last of its axis: 4 classes per axis, 64
// masks).
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
    // does the node of size dim at (ox, oy, oz) meet the box?
    bool overlaps(int ox, int oy, int oz, int dim) const
    {
        return ox + dim - 1 >= lo && ox <= hi && oy + dim - 1 >= lo && oy <= hi && oz + dim - 1 >= lo && oz <= hi;
    }
    int64_t nodes(int dim) const { const int64_t c = (floor_to(hi, dim) - floor_to(lo, dim)) / dim + 1; return c * c * c; }   // of size dim, in the tree
};

struct Writer {
    Out o;
    int n = 0, n_grids = 0, written = 0;
    uint32_t compression = 0;
    std::map<int, std::vector<unsigned char>> zero_values;   // leaf path: the value bytes of a leaf of na zeros, by na
};

// every writer of the call receives the same bytes
struct Fan {
    Writer* const* w;
    int n;
    void raw(const void* p, size_t len) const { for (int i = 0; i < n; ++i) w[i]->o.raw(p, len); }
};

// The walk over the tree of the box: root children in ascending (x,y,z) origin order (std::map<Coord>, math/Coord.h:180-185),
// their 128^3 nodes and the leaves of those by ascending offset.  In the topology pass it writes every root child's origin and
// every internal node's child mask and (background) tiles.  What is written for a leaf, in either pass, is the caller's:
// leaf(i, j, k), the leaf's indices among the grid's leaves, and end_node() behind the last leaf of each 128^3 node.
template <typename Leaf, typename EndNode>
void walk_tree(const Fan& f, const LeafGeom& g, bool topology, uint32_t compression, Leaf leaf, EndNode end_node)
{
    for (int rx = floor_to(g.lo, INT2); rx <= g.hi; rx += INT2)
        for (int ry = floor_to(g.lo, INT2); ry <= g.hi; ry += INT2)
            for (int rz = floor_to(g.lo, INT2); rz <= g.hi; rz += INT2) {
                if (topology) {
                    const int32_t org[3] = {rx, ry, rz};
                    f.raw(org, sizeof(org));
                    std::vector<uint64_t> cm(32 * 32 * 32 / 64, 0);  // child mask of the 4096^3 node: 32^3 slots of 128^3
                    for (int a = 0; a < 32; ++a)
                        for (int b = 0; b < 32; ++b)
                            for (int c = 0; c < 32; ++c)
                                if (g.overlaps(rx + a * INT1, ry + b * INT1, rz + c * INT1, INT1)) {
                                    const int n = (a << 10) + (b << 5) + c;
                                    cm[n >> 6] |= 1ull << (n & 63);
                                }
                    f.raw(cm.data(), cm.size() * 8);
                    for (int i = 0; i < f.n; ++i) background_tiles(f.w[i]->o, cm.size() * 8, compression);
                }
                for (int a = 0; a < 32; ++a)
                    for (int b = 0; b < 32; ++b)
                        for (int c = 0; c < 32; ++c) {
                            const int ix = rx + a * INT1, iy = ry + b * INT1, iz = rz + c * INT1;
                            if (!g.overlaps(ix, iy, iz, INT1)) continue;
                            if (topology) {
                                uint64_t cm[64] = {};  // 16^3 slots of 8^3
                                for (int p = 0; p < 16; ++p)
                                    for (int q = 0; q < 16; ++q)
                                        for (int r = 0; r < 16; ++r)
                                            if (g.overlaps(ix + p * LEAF, iy + q * LEAF, iz + r * LEAF, LEAF)) {
                                                const int n = (p << 8) + (q << 4) + r;
                                                cm[n >> 6] |= 1ull << (n & 63);
                                            }
                                f.raw(cm, sizeof(cm));
                                for (int i = 0; i < f.n; ++i) background_tiles(f.w[i]->o, sizeof(cm), compression);
                            }
                            for (int p = 0; p < 16; ++p)
                                for (int q = 0; q < 16; ++q)
                                    for (int r = 0; r < 16; ++r) {
                                        const int lx = ix + p * LEAF, ly = iy + q * LEAF, lz = iz + r * LEAF;
                                        if (g.overlaps(lx, ly, lz, LEAF)) leaf((lx - g.L0) / LEAF, (ly - g.L0) / LEAF, (lz - g.L0) / LEAF);
                                    }
                            end_node();
                        }
            }
}

// ---- the grid from a dense array (fluid_vdb_append) ----------------------------------------------------------------------------
// One leaf of the buffers pass: its active values and (ZIP) the zipToStream framing of them, prepared off the output stream so that
// the leaves of a 128^3 node can be compressed on several host threads (zlib at the library's default level costs ~20 us per leaf:
// 80 ms for a 121^3 grid on one thread, written twice per step by the driver); the bytes are those of the serial path, in the
// same order.
struct LeafJob {
    int i, j, k, cls;
    int na;
    float act[512];
    int64_t head;                       // zip: the int64 in front (compressed size, or -raw size)
    std::vector<unsigned char> z;       // zip: the compressed bytes (empty: the raw values follow)
};
// zbuf: the calling thread's zip_frame buffer, so a job keeps its compressed bytes only
void prepare_leaf(const LeafGeom& G, const float* grid, LeafJob& j, uint32_t compression, std::vector<unsigned char>& zbuf)
{
    j.cls = G.leaf_class(j.i, j.j, j.k);
    const int cx = j.cls >> 4, cy = (j.cls >> 2) & 3, cz = j.cls & 3;
    const int bx = G.L0 + LEAF * j.i - G.lo, by = G.L0 + LEAF * j.j - G.lo, bz = G.L0 + LEAF * j.k - G.lo;   // the leaf's origin in the array
    j.na = 0;
    for (int x = G.a0[cx]; x <= G.a1[cx]; ++x)
        for (int y = G.a0[cy]; y <= G.a1[cy]; ++y)
            for (int z = G.a0[cz]; z <= G.a1[cz]; ++z) j.act[j.na++] = grid[((size_t)(bx + x) * G.n + (by + y)) * G.n + (bz + z)];
    j.head = (compression & COMPRESS_ZIP) ? zip_frame(j.act, (size_t)j.na * sizeof(float), zbuf) : 0;
    if (j.head > 0) j.z.assign(zbuf.begin(), zbuf.begin() + j.head);
}
void flush_leaves(Out& o, const LeafGeom& G, const float* grid, std::vector<LeafJob>& jobs, uint32_t compression)
{
    const size_t n = jobs.size();
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : (nt > 16 ? 16 : nt);
    if (n < 64 || !(compression & COMPRESS_ZIP)) nt = 1;
    auto share = [&](unsigned t) {
        std::vector<unsigned char> zbuf;
        for (size_t i = t; i < n; i += nt) prepare_leaf(G, grid, jobs[i], compression, zbuf);
    };
    if (nt == 1) {
        share(0);
    } else {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; ++t) th.emplace_back(share, t);
        for (auto& x : th) x.join();
    }
    for (auto& j : jobs) {
        o.raw(G.mask[j.cls], sizeof(G.mask[j.cls]));
        o.put<int8_t>(NO_MASK_OR_INACTIVE_VALS);  // inactive voxels hold the background
        if (compression & COMPRESS_ZIP) o.put<int64_t>(j.head);
        if (j.head > 0) o.raw(j.z.data(), (size_t)j.head);
        else o.raw(j.act, (size_t)j.na * sizeof(float));
    }
    jobs.clear();
}

void write_tree(Writer& w, const LeafGeom& G, const float* grid, bool buffers)
{
    Writer* const one = &w;
    std::vector<LeafJob> jobs;
    walk_tree(Fan{&one, 1}, G, !buffers, w.compression,
              [&](int i, int j, int k) {
                  if (!buffers) {
                      const int cls = G.leaf_class(i, j, k);
                      w.o.raw(G.mask[cls], sizeof(G.mask[cls]));
                      return;
                  }
                  jobs.emplace_back();   // (the leaves of this 128^3 node are written together, at its end)
                  jobs.back().i = i; jobs.back().j = j; jobs.back().k = k;
              },
              [&] { if (buffers) flush_leaves(w.o, G, grid, jobs, w.compression); });
}

int writer_open(Writer& w, const char* path, int32_t n, int32_t n_grids, int32_t compression)
{
    w.n = n; w.n_grids = n_grids; w.written = 0;
    w.compression = (uint32_t)compression;
    w.o.f = fopen(path, "wb");
    if (!w.o.f) return FLUID_ERR_ARG;
    file_header(w.o, n_grids);
    return FLUID_OK;
}

// grid_head of the writer's next grid: unnamed, so "\x1e<k>" (io/Archive.cc:1196-1206); every voxel of the box is active
size_t density_head(Writer& w, const LeafGeom& G)
{
    const int32_t bmin[3] = {G.lo, G.lo, G.lo}, bmax[3] = {G.hi, G.hi, G.hi};
    const int64_t mem = tree_mem_bytes(G.nodes(INT2), G.nodes(INT1), G.nodes(LEAF));
    return grid_head(w.o, std::string("\x1e") + std::to_string(w.written), w.compression,
                     file_stats(w.compression, bmin, bmax, mem, (int64_t)G.n * G.n * G.n), 1.0, 0.0f, (uint32_t)G.nodes(INT2));
}

int writer_append(Writer& w, const float* grid)
{
    if (w.written >= w.n_grids) return FLUID_ERR_STATE;
    Out& o = w.o;
    const LeafGeom G(w.n);
    const size_t off = density_head(w, G);
    write_tree(w, G, grid, false);
    o.patch64(off + 8, (int64_t)o.pos());   // block position
    write_tree(w, G, grid, true);
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
// work: a leaf the list does not name holds zeros only, so its value bytes are a constant of its active-voxel count; the listed
// leaves are gathered and zipped once for all writers of the call.

// the bytes that follow a leaf's metadata byte in the buffers pass, for its na active values
void value_bytes(const float* act, int na, uint32_t compression, std::vector<unsigned char>& out, std::vector<unsigned char>& z)
{
    const unsigned char* raw = (const unsigned char*)act;
    const size_t n = (size_t)na * sizeof(float);
    if (!(compression & COMPRESS_ZIP)) { out.insert(out.end(), raw, raw + n); return; }
    const int64_t head = zip_frame(act, n, z);
    out.insert(out.end(), (const unsigned char*)&head, (const unsigned char*)&head + 8);
    if (head > 0) out.insert(out.end(), z.begin(), z.begin() + head);
    else out.insert(out.end(), raw, raw + n);
}

struct Span { const unsigned char* p; size_t n; };

void write_tree_leaves(const Fan& f, const LeafGeom& G, bool buffers, uint32_t compression, const std::vector<int>& table,
                       const std::vector<Span>& listed, const Span zero[64])
{
    const int8_t meta_byte = NO_MASK_OR_INACTIVE_VALS;
    std::vector<unsigned char> chunk;
    auto add = [&](const void* p, size_t len) { chunk.insert(chunk.end(), (const unsigned char*)p, (const unsigned char*)p + len); };
    walk_tree(f, G, !buffers, compression,
              [&](int i, int j, int k) {
                  const int cls = G.leaf_class(i, j, k);
                  add(G.mask[cls], sizeof(G.mask[cls]));
                  if (!buffers) return;
                  add(&meta_byte, 1);
                  const int t = table[((size_t)i * G.nl + j) * G.nl + k];
                  const Span& s = t >= 0 ? listed[(size_t)t] : zero[cls];
                  add(s.p, s.n);
              },
              [&] {   // the leaves of this 128^3 node, to every writer at once
                  f.raw(chunk.data(), chunk.size());
                  chunk.clear();
              });
}

int append_leaves(Writer* const* ws, int nw, const fluid_leaf_grid_t* g)
{
    const uint32_t compression = ws[0]->compression;
    for (int i = 0; i < nw; ++i)
        if (ws[i]->n != g->n || ws[i]->compression != compression) return FLUID_ERR_ARG;
    int rc = check_list(g);
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
    for (int i = 0; i < nw; ++i) off[(size_t)i] = density_head(*ws[i], G);
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
    const int rc = check_list(g);
    if (rc) return rc;
    memset(dense, 0, (size_t)g->n * g->n * g->n * sizeof(float));
    scatter_leaves(g, [&](size_t l, int off, size_t c) { dense[c] = g->values[512 * l + off]; });
    return FLUID_OK;
}

// The k-way merge of the parts' lists (merge_walk), run twice: the first pass counts and checks and writes nothing, the second
// writes.  A leaf listed by one part is copied; one listed by several is OR-ed as bit patterns — exact, because a voxel is owned by
// one part and +0 in the others, which the first pass verifies.
int64_t fluid_leaf_grids_merge(const fluid_leaf_grid_t* parts, int32_t n_parts, int64_t cap_leaves, int32_t* origin, float* values)
{
    if (!parts || n_parts < 1 || (origin == nullptr) != (values == nullptr)) return -FLUID_ERR_ARG;
    for (int p = 0; p < n_parts; ++p)
        if (check_list(&parts[p]) != FLUID_OK || parts[p].n != parts[0].n) return -FLUID_ERR_ARG;
    auto n_leaves_of = [&](int p) { return parts[p].n_leaves; };
    auto origin_of = [&](int p, long l) { return org_of(&parts[p], l); };
    int64_t count = 0;
    for (int pass = 0; pass < (origin ? 2 : 1); ++pass) {
        if (pass == 1 && count > cap_leaves) return -FLUID_ERR_ARG;
        count = 0;
        const bool check = pass == 0;
        const bool merged = merge_walk(n_parts, n_leaves_of, origin_of, [&, check](const Org& o, int n_in, const int32_t* part, const int32_t* leaf) {
            uint32_t acc[512];
            memcpy(acc, parts[part[0]].values + 512 * (size_t)leaf[0], sizeof acc);
            for (int t = 1; t < n_in; ++t) {
                const float* v = parts[part[t]].values + 512 * (size_t)leaf[t];
                for (int i = 0; i < 512; ++i) {
                    uint32_t b;
                    memcpy(&b, v + i, sizeof b);
                    if (check && b && acc[i]) return false;   // two parts claim the voxel
                    acc[i] |= b;
                }
            }
            if (pass == 1) {
                memcpy(origin + 3 * (size_t)count, &o, sizeof o);
                memcpy(values + 512 * (size_t)count, acc, sizeof acc);
            }
            count++;
            return true;
        });
        if (!merged) return -FLUID_ERR_ARG;
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
    int rc = check_list(g);   // before the file is created
    if (rc) return rc;
    fluid_vdb_writer_t* h = nullptr;
    rc = fluid_vdb_open(path, g->n, 1, compression, &h);
    if (rc) return rc;
    rc = fluid_vdb_append_leaves(&h, 1, g);
    const int rc2 = fluid_vdb_close(h);
    return rc ? rc : rc2;
}

}  // extern "C"
