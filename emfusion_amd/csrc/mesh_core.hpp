// mesh_core.hpp -- what the two consumers of the marching-cubes geometry share: the cube / corner /
// edge conventions of the reference (TSDF.cu:872-1096) and its vertexInterp.  lifecycle.hip streams
// the edge vertices into order statistics (updateObj), meshing.hip emits the mesh itself.
#pragma once

#include "common.hpp"

namespace emf_hip {

struct MeshSource {
    const float* tsdf;
    const float* weights;
    const uint8_t* fg;  // fgVolMask or nullptr
    I3 n;
    float voxelSize;
};

// vertexInterp's decision (TSDF.cu:909-920; the comparisons are against the double literal 0.00001): 1 = the first
// corner's value outright, 2 = the second's (its three early returns), 0 = a1 + mu * (a2 - a1).  Shared by everything
// that is interpolated along an edge: positions and normals (vertex_interp), vertex colours.
__device__ __forceinline__ int vertex_interp_mu(float v1, float v2, float& mu) {
    mu = 0.f;
    if (static_cast<double>(fabsf(v1)) < 0.00001) return 1;
    if (static_cast<double>(fabsf(v2)) < 0.00001) return 2;
    if (static_cast<double>(fabsf(v1 - v2)) < 0.00001) return 1;
    mu = -v1 / (v2 - v1);
    return 0;
}

__device__ __forceinline__ V3 vertex_interp(const V3& p1, const V3& p2, float v1, float v2) {
    float mu;
    const int take = vertex_interp_mu(v1, v2, mu);
    if (take == 1) return p1;
    if (take == 2) return p2;
    const V3 d = v3(p2.x - p1.x, p2.y - p1.y, p2.z - p1.z);  // p1 + mu * (p2 - p1)
    return p1 + d * mu;
}

// The colour of the vertex on an edge whose endpoints hold the voxels c[0], c[1] (R, G, B in 1/256 levels, Wc) and the
// values v1, v2: an uncoloured endpoint (Wc == 0) contributes the other endpoint's colour; both: black.  Interpolated
// like the position, with contraction off whatever the build says, then rounded to u8.
__device__ __forceinline__ void edge_colour(ushort4 c0, ushort4 c1, float v1, float v2, uint8_t* o) {
#pragma clang fp contract(off)
    if (c0.w == 0) c0 = c1;
    if (c1.w == 0) c1 = c0;
    const bool none = c0.w == 0;
    float mu;
    const int take = vertex_interp_mu(v1, v2, mu);
    const unsigned short a[3] = {c0.x, c0.y, c0.z}, b[3] = {c1.x, c1.y, c1.z};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float c1f = static_cast<float>(a[j]) / 256.f, c2f = static_cast<float>(b[j]) / 256.f;
        const float v = take == 1 ? c1f : (take == 2 ? c2f : c1f + mu * (c2f - c1f));
        o[j] = none ? 0 : static_cast<uint8_t>(fminf(fmaxf(rintf(v), 0.f), 255.f));
    }
}

// corner i of cube (x, y, z) in the reference's numbering (TSDF.cu:896-903): x + (i ^ (i >> 1)) & 1,
// z + (i >> 1) & 1, y + (i >> 2) & 1
__device__ __forceinline__ void cube_corner(int i, int& dx, int& dy, int& dz) {
    dx = ((i & 1) ^ ((i >> 1) & 1));
    dz = (i >> 1) & 1;
    dy = (i >> 2) & 1;
}

// the corners joined by edge e (bit e of the reference's edgeTable[cls] is set iff their signs differ)
__device__ __forceinline__ unsigned active_edges(unsigned cls) {
    constexpr int e0[12] = {0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3};
    constexpr int e1[12] = {1, 2, 3, 0, 5, 6, 7, 4, 4, 5, 6, 7};
    unsigned m = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) m |= (((cls >> e0[e]) ^ (cls >> e1[e])) & 1u) << e;
    return m;
}

}  // namespace emf_hip
