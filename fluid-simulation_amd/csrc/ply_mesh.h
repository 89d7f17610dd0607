// The body of fluid_write_ply_mesh, fluid_write_ply_mesh_attr and fluid_write_ply_mesh_ex (mesh_host.cpp), which check their own
// arguments first: binary little-endian PLY, a vertex record of 12 bytes of scaled position, 12 more of the normal and 12 more of
// the scaled velocity where given; faces are the quads, or the triangles where given.  And the body of fluid_mesh_triangles
// (include/fluid_hip.h, "normals and triangles"), whose cut of a quad is mesh_def.h's.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fluid_hip.h"
#include "mesh_def.h"

namespace {

// the body of fluid_mesh_triangles
inline int64_t mesh_triangles(const fluid_mesh_t* m, int64_t cap_triangles, uint32_t* triangles)
{
    if (!m || m->n_vertices < 0 || m->n_quads < 0 || m->n_quads > 0x7fffffffLL) return -FLUID_ERR_ARG;
    if ((m->n_vertices > 0 && !m->vertices) || (m->n_quads > 0 && !m->quads)) return -FLUID_ERR_ARG;
    for (int64_t i = 0; i < 4 * m->n_quads; ++i)
        if ((int64_t)m->quads[i] >= m->n_vertices) return -FLUID_ERR_ARG;
    if (!triangles) return 2 * m->n_quads;
    if (2 * m->n_quads > cap_triangles) return -FLUID_ERR_ARG;
    // quad i = (a, b, c, d) -> triangles 2i and 2i + 1
    for (int64_t i = 0; i < m->n_quads; ++i) {
        const uint32_t* q = m->quads + 4 * i;
        const float* V = m->vertices;
        mdef::quad_triangles(q, V + 3 * (size_t)q[0], V + 3 * (size_t)q[1], V + 3 * (size_t)q[2], V + 3 * (size_t)q[3], triangles + 6 * i);
    }
    return 2 * m->n_quads;
}

// with_velocity: vx / vy / vz in the header and velocity[3 i ..] * velocity_scale in vertex i's record; normals: nx / ny / nz between
// the position and the velocity, unscaled; triangles (3 uint32 each, 2 per quad): the faces, instead of the quads
inline int write_ply(const char* path, const fluid_mesh_t* m, float voxel_size, bool with_velocity, const float* velocity, float velocity_scale,
                     const float* normals = nullptr, const uint32_t* triangles = nullptr)
{
    for (int64_t i = 0; i < 4 * m->n_quads; ++i)
        if ((int64_t)m->quads[i] >= m->n_vertices) return FLUID_ERR_ARG;
    for (int64_t i = 0; triangles && i < 6 * m->n_quads; ++i)
        if ((int64_t)triangles[i] >= m->n_vertices) return FLUID_ERR_ARG;
    FILE* f = fopen(path, "wb");
    if (!f) return FLUID_ERR_ARG;
    bool ok = fprintf(f,
                      "ply\nformat binary_little_endian 1.0\nelement vertex %lld\nproperty float x\nproperty float y\nproperty float z\n"
                      "%s%selement face %lld\nproperty list uchar uint vertex_indices\nend_header\n",
                      (long long)m->n_vertices, normals ? "property float nx\nproperty float ny\nproperty float nz\n" : "",
                      with_velocity ? "property float vx\nproperty float vy\nproperty float vz\n" : "", (long long)(triangles ? 2 * m->n_quads : m->n_quads)) > 0;
    std::vector<char> buf;
    buf.reserve((size_t)1 << 20);
    auto flush = [&] {
        if (!buf.empty() && fwrite(buf.data(), 1, buf.size(), f) != buf.size()) ok = false;
        buf.clear();
    };
    for (int64_t i = 0; ok && i < m->n_vertices; ++i) {
        float rec[9];
        int k = 3;
        for (int a = 0; a < 3; ++a) rec[a] = m->vertices[3 * i + a] * voxel_size;
        if (normals)
            for (int a = 0; a < 3; ++a) rec[k++] = normals[3 * i + a];
        if (with_velocity)
            for (int a = 0; a < 3; ++a) rec[k++] = velocity[3 * i + a] * velocity_scale;
        const char* c = (const char*)rec;
        buf.insert(buf.end(), c, c + 4 * k);
        if (buf.size() >= ((size_t)1 << 20) - 32) flush();
    }
    for (int64_t i = 0; ok && triangles && i < 2 * m->n_quads; ++i) {
        buf.push_back((char)3);
        const char* c = (const char*)(triangles + 3 * i);
        buf.insert(buf.end(), c, c + 12);
        if (buf.size() >= ((size_t)1 << 20) - 32) flush();
    }
    for (int64_t i = 0; ok && !triangles && i < m->n_quads; ++i) {
        buf.push_back((char)4);
        const char* c = (const char*)(m->quads + 4 * i);
        buf.insert(buf.end(), c, c + 16);
        if (buf.size() >= ((size_t)1 << 20) - 32) flush();
    }
    flush();
    const int frc = fclose(f);
    if (ok && frc == 0) return FLUID_OK;
    remove(path);   // a short write leaves no partial file behind
    return FLUID_ERR_ARG;   // (the ABI has no code of its own for I/O: an unwritable path is a bad argument, as in the .vdb writers)
}

}  // namespace
