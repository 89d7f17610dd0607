// The body of fluid_write_ply_mesh (mesh_host.cpp) and fluid_write_ply_mesh_attr (mesh_attr_host.cpp), which check their own
// arguments first: binary little-endian PLY, a vertex record of 12 bytes of scaled position, or 24 with the scaled velocity.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fluid_hip.h"

namespace {

// with_velocity: vx / vy / vz in the header and velocity[3 i ..] * velocity_scale behind vertex i's position
inline int write_ply(const char* path, const fluid_mesh_t* m, float voxel_size, bool with_velocity, const float* velocity, float velocity_scale)
{
    for (int64_t i = 0; i < 4 * m->n_quads; ++i)
        if ((int64_t)m->quads[i] >= m->n_vertices) return FLUID_ERR_ARG;
    FILE* f = fopen(path, "wb");
    if (!f) return FLUID_ERR_ARG;
    bool ok = fprintf(f,
                      "ply\nformat binary_little_endian 1.0\nelement vertex %lld\nproperty float x\nproperty float y\nproperty float z\n"
                      "%selement face %lld\nproperty list uchar uint vertex_indices\nend_header\n",
                      (long long)m->n_vertices, with_velocity ? "property float vx\nproperty float vy\nproperty float vz\n" : "", (long long)m->n_quads) > 0;
    std::vector<char> buf;
    buf.reserve((size_t)1 << 20);
    auto flush = [&] {
        if (!buf.empty() && fwrite(buf.data(), 1, buf.size(), f) != buf.size()) ok = false;
        buf.clear();
    };
    for (int64_t i = 0; ok && i < m->n_vertices; ++i) {
        float rec[6];
        for (int a = 0; a < 3; ++a) rec[a] = m->vertices[3 * i + a] * voxel_size;
        if (with_velocity)
            for (int a = 0; a < 3; ++a) rec[3 + a] = velocity[3 * i + a] * velocity_scale;
        const char* c = (const char*)rec;
        buf.insert(buf.end(), c, c + (with_velocity ? 24 : 12));
        if (buf.size() >= ((size_t)1 << 20) - 32) flush();
    }
    for (int64_t i = 0; ok && i < m->n_quads; ++i) {
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
