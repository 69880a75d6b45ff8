// voxel_rays.hip -- voxel rays: straight integer walks through a box of class bytes, each stopped by the first voxel
// that blocks, and their sums per group of rays (include/emf_hip.h "Voxel rays").
//
// Linear index i = (z * ny + y) * nx + x < 2^31.  A ray a -> b makes d_x + d_y + d_z face steps; the next step goes
// along the axis that has steps left and the smallest crossing parameter (2 i_k + 1) / (2 d_k), compared by
// cross-multiplication (products below 2^26), ties to the lower axis.
//   k_vr_cast   one lane per ray, 256 rays per workgroup.  A lane's loop runs d_x + d_y + d_z <= 3 * EMF_RAY_MAX_DELTA
//               times at most, so a wave runs as long as its longest ray, whatever the memory holds.  The axis is
//               chosen by selects, not branches: the lanes of a wave diverge only where their rays end.  A voxel is
//               tested against the box before its class byte is read, and d2 only where the class passed.  After
//               the loop the whole wave meets again: the six group quantities go through run_scan of wave_ops.hpp
//               (rays of a group are consecutive, so a group is one run of lanes), and the last lane
//               of each run adds the run's sums to the group's record with one integer atomic per non-zero quantity.
//               Integer sums: the records do not depend on the order of waves or workgroups.
// The group records are zeroed by a memset on the stream before the launch.  No float, no LDS, no scratch memory.
#include "common.hpp"
#include "wave_ops.hpp"

namespace emf_hip {
namespace {

constexpr int kVrBlock = 256;

struct RayArgs {
    const uint8_t* classes;
    const int32_t* d2;  // NULL: no gate
    const int32_t* from;
    const int32_t* to;
    emf_ray_result_t* results;  // or NULL
    emf_ray_group_t* groups;    // or NULL
    int nx, ny, nz;
    int minD2;
    unsigned passMask, countMask;
    int n, group;
};

__global__ __launch_bounds__(kVrBlock) void k_vr_cast(const RayArgs a) {
    const int lane = threadIdx.x & 63;
    const long long i = static_cast<long long>(blockIdx.x) * kVrBlock + threadIdx.x;
    const bool live = i < a.n;
    int stop = EMF_DF_NONE, steps = 0;
    unsigned counted = 0u, status = EMF_RAY_INVALID;
    unsigned long long weighted = 0ull;
    if (live) {
        const int ax = a.from[3 * i], ay = a.from[3 * i + 1], az = a.from[3 * i + 2];
        const long long ex = static_cast<long long>(a.to[3 * i]) - ax, ey = static_cast<long long>(a.to[3 * i + 1]) - ay,
                        ez = static_cast<long long>(a.to[3 * i + 2]) - az;
        const long long lx = ex < 0 ? -ex : ex, ly = ey < 0 ? -ey : ey, lz = ez < 0 ? -ez : ez;
        if (ax < 0 || ax >= a.nx || ay < 0 || ay >= a.ny || az < 0 || az >= a.nz) {
            status = EMF_RAY_OUTSIDE;
        } else if (lx <= EMF_RAY_MAX_DELTA && ly <= EMF_RAY_MAX_DELTA && lz <= EMF_RAY_MAX_DELTA) {
            const int dx = static_cast<int>(lx), dy = static_cast<int>(ly), dz = static_cast<int>(lz);
            const int sx = ex < 0 ? -1 : 1, sy = ey < 0 ? -1 : 1, sz = ez < 0 ? -1 : 1;
            const int plane = a.nx * a.ny;
            const int total = min(dx + dy + dz, 3 * EMF_RAY_MAX_DELTA);
            const bool gate = a.d2 != nullptr && a.minD2 > 0;
            int ix = 0, iy = 0, iz = 0, x = ax, y = ay, z = az;
            int lin = az * plane + ay * a.nx + ax;
            status = EMF_RAY_REACHED;
            for (int k = 0; k < total; ++k) {
                const int px = 2 * ix + 1, py = 2 * iy + 1, pz = 2 * iz + 1;
                const bool hx = ix < dx, hy = iy < dy, hz = iz < dz;
                const bool xBeforeY = hx && (!hy || px * dy <= py * dx);
                const bool xBeforeZ = !hz || px * dz <= pz * dx;
                const bool yBeforeZ = hy && (!hz || py * dz <= pz * dy);
                const int axis = xBeforeY ? (xBeforeZ ? 0 : 2) : (yBeforeZ ? 1 : 2);
                const int mx = axis == 0, my = axis == 1, mz = axis == 2;
                ix += mx;
                iy += my;
                iz += mz;
                x += mx * sx;
                y += my * sy;
                z += mz * sz;
                if (x < 0 || x >= a.nx || y < 0 || y >= a.ny || z < 0 || z >= a.nz) {
                    status = EMF_RAY_LEFT;
                    break;
                }
                lin += mx * sx + my * sy * a.nx + mz * sz * plane;
                const unsigned c = a.classes[lin];
                const unsigned bit = c <= 2u ? 1u << c : 0u;
                bool pass = (bit & a.passMask) != 0u;
                if (pass && gate) pass = a.d2[lin] >= a.minD2;
                if (!pass) {
                    status = EMF_RAY_BLOCKED;
                    stop = lin;
                    break;
                }
                ++steps;
                if (bit & a.countMask) {
                    ++counted;
                    weighted += static_cast<unsigned>(ix * ix + iy * iy + iz * iz);
                }
            }
        }
        if (a.results != nullptr) {
            emf_ray_result_t r;
            r.stop = stop;
            r.steps = steps;
            r.counted = counted;
            r.status = status;
            r.weighted = weighted;
            a.results[i] = r;
        }
    }
    if (a.groups == nullptr) return;  // wave-uniform
    // every lane of the wave is here: the lanes past the list form a run of their own that adds nothing.  The group
    // number ascends with the lane, so it is the run number (wave_ops.hpp)
    const int run = live ? static_cast<int>(i / a.group) : -1;
    const unsigned long long sumCounted = run_scan<OpAdd, unsigned long long>(counted, lane, run);
    const unsigned long long sumWeighted = run_scan<OpAdd>(weighted, lane, run);
    const unsigned sumReached = run_scan<OpAdd>(live && status == EMF_RAY_REACHED ? 1u : 0u, lane, run);
    const unsigned sumBlocked = run_scan<OpAdd>(live && status == EMF_RAY_BLOCKED ? 1u : 0u, lane, run);
    const unsigned sumLeft = run_scan<OpAdd>(live && status == EMF_RAY_LEFT ? 1u : 0u, lane, run);
    const unsigned sumInvalid = run_scan<OpAdd>(live && status >= EMF_RAY_OUTSIDE ? 1u : 0u, lane, run);
    if (!run_is_last(run, lane) || !live) return;
    emf_ray_group_t* g = a.groups + run;
    if (sumCounted) atomicAdd(reinterpret_cast<unsigned long long*>(&g->counted), sumCounted);
    if (sumWeighted) atomicAdd(reinterpret_cast<unsigned long long*>(&g->weighted), sumWeighted);
    if (sumReached) atomicAdd(&g->reached, sumReached);
    if (sumBlocked) atomicAdd(&g->blocked, sumBlocked);
    if (sumLeft) atomicAdd(&g->left, sumLeft);
    if (sumInvalid) atomicAdd(&g->invalid, sumInvalid);
}

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

int emf_hip_castVoxelRays(const uint8_t* classes, const int32_t size[3], const int32_t* d2, int32_t min_d2, uint32_t pass_mask,
                          uint32_t count_mask, const int32_t* from, const int32_t* to, int32_t n, emf_ray_result_t* results,
                          int32_t group, emf_ray_group_t* groups, emf_stream_t stream) {
    if (!size) return fail(EMF_E_ARG, "castVoxelRays: size is NULL");
    for (int i = 0; i < 3; ++i) {  // the limits of the distance field
        if (size[i] < 1) return fail(EMF_E_ARG, "castVoxelRays: box axis %d has %d voxels", i, size[i]);
        if (size[i] > EMF_DF_MAX_AXIS)
            return fail(EMF_E_LIMIT, "castVoxelRays: box axis %d has %d voxels, above %d", i, size[i], EMF_DF_MAX_AXIS);
    }
    const unsigned long long voxels = static_cast<unsigned long long>(size[0]) * size[1] * static_cast<unsigned long long>(size[2]);
    if (voxels > 0x7fffffffull) return fail(EMF_E_LIMIT, "castVoxelRays: a box of %llu voxels, above 2^31 - 1", voxels);
    if (pass_mask > 7u || count_mask > 7u)
        return fail(EMF_E_ARG, "castVoxelRays: pass_mask %u or count_mask %u outside 0 .. 7", pass_mask, count_mask);
    if (n < 0 || group < 0) return fail(EMF_E_ARG, "castVoxelRays: %d rays in groups of %d", n, group);
    if (!classes || !from || !to) return fail(EMF_E_ARG, "castVoxelRays: classes, from or to is NULL");
    if ((group > 0) != (groups != nullptr)) return fail(EMF_E_ARG, "castVoxelRays: group > 0 and the group records go together");
    if (!results && !groups) return fail(EMF_E_ARG, "castVoxelRays: neither results nor groups");
    if ((reinterpret_cast<uintptr_t>(d2) | reinterpret_cast<uintptr_t>(from) | reinterpret_cast<uintptr_t>(to)) & 3u ||
        (reinterpret_cast<uintptr_t>(results) | reinterpret_cast<uintptr_t>(groups)) & 7u)
        return fail(EMF_E_ARG, "castVoxelRays: misaligned arrays");
    if (n == 0) return EMF_OK;
    const hipStream_t s = as_stream(stream);
    if (groups) {
        const size_t nGroups = (static_cast<size_t>(n) + group - 1) / group;
        const hipError_t e = hipMemsetAsync(groups, 0, nGroups * sizeof(emf_ray_group_t), s);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_error("castVoxelRays: memset: %s", hipGetErrorString(e));
            return static_cast<int>(e);
        }
    }
    const RayArgs a{classes, d2, from, to, results, groups, size[0], size[1], size[2], min_d2, pass_mask, count_mask, n, group};
    hipLaunchKernelGGL(k_vr_cast, dim3(ceil_div(static_cast<size_t>(n), kVrBlock)), dim3(kVrBlock), 0, s, a);
    return launch_status("castVoxelRays");
}

}  // extern "C"
