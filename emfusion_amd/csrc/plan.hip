// plan.hip -- path planning: the cost-to-go field through the traversable voxels of a box of class bytes, and the
// paths from any number of goals back to a start (include/emf_hip.h "Planning").
//
// Linear index i = (z * ny + y) * nx + x < 2^29.  The field is the unique fixed point of
// cost[v] = min(cost[v], cost[n] + w(n, v)) over the traversable set T, so any order of relaxations that runs until
// nothing changes gives the same bytes.  A tile is kTx x kTy x kTz voxels; tiles are numbered (tz * tilesY + ty) *
// tilesX + tx.  The scratch holds two byte flags per tile ("active in a round of parity 0 / 1") and one activity
// counter per round of a batch.
//   k_pl_init   one wave per row.  cost = BLOCKED outside T, UNREACHED inside it, 0 at a used seed; the tiles that hold
//               a used seed or have it in their halo get their parity-0 flag; used seeds counted.  The seeds are a small device array every wave reads.
//   k_pl_relax  one workgroup per tile; a tile whose flag of this round's parity is clear leaves at once.  The tile's
//               costs and a one-voxel halo go into LDS (BLOCKED outside the box), the tile is relaxed there in sweeps
//               until a sweep changes nothing or kSweeps are done, the voxels that changed are written back by their
//               own thread -- each voxel is written by its own tile only, no atomics on the field -- and a changed
//               voxel on the tile's shell sets the next-parity flag of the tiles that have it in their halo.  A tile
//               still changing at the bound sets its own.  Thread 0 clears the tile's flag of this parity and adds
//               one to the round's activity counter.
//               VISIBILITY.  Nothing here relies on one workgroup seeing another's stores inside a launch: the L2s
//               of the eight XCDs are not coherent with each other within a kernel and a CU's L1 is not refreshed by
//               another CU's stores.  Costs only ever decrease, so a stale halo word is a LARGER value than the
//               current one: an upper bound that is never wrong, only late.  Whoever lowers a shell voxel flags the
//               neighbours for the NEXT launch, and at a launch boundary all stores are visible.  The flags are plain
//               byte stores of the value 1 (all writers store the same) into the buffer no tile reads this round.
//               After round k the k cheapest voxels of T are final (a voxel's predecessor on its cheapest path was
//               final a round before and either shares its tile or flagged it), so rounds <= |T| + 1.
//   k_pl_finish counts the voxels with a finite cost and writes the host loop's two counters
//   k_pl_paths  one wave per goal; lanes 0..25 test the 26 neighbours in ascending linear-index order, the lowest
//               set bit of the __ballot is the step.
// The host loop (emf_hip_planCost) enqueues rounds in batches of kBatch, reads the batch's activity counters back and
// stops at the first round in which no tile was active.  No cooperative launch, no grid barrier, no waiting between
// workgroups; every device loop is bounded by a constant or an argument.  No index leaves its array: a neighbour is
// tested against the box before it is read, a tile against the tile grid before it is flagged.
#include "common.hpp"
#include "wave_ops.hpp"

namespace emf_hip {
namespace {

constexpr int kTx = 32, kTy = 8, kTz = 8;  // the integration tile (DESIGN 5.20 has the figure of 8 x 8 x 8)
constexpr int kPlBlock = 256;
constexpr int kPerThread = kTx * kTy * kTz / kPlBlock;  // voxels of a tile per thread
constexpr int kHx = kTx + 2, kHy = kTy + 2, kHz = kTz + 2;
constexpr int kHalo = kHx * kHy * kHz;
constexpr int kSweeps = kTx + kTy + kTz;  // a straight run through an open tile needs no more
constexpr int kBatch = 16;                // rounds enqueued between two looks at the activity counters
constexpr unsigned kUnreached = EMF_PLAN_UNREACHED, kBlocked = EMF_PLAN_BLOCKED;
constexpr unsigned long long kMaxVoxels = 1ull << 29;

static_assert(kTx * kTy * kTz % kPlBlock == 0 && kPerThread >= 1, "whole voxels per thread");

struct PlArgs {
    uint8_t* flags;    // 2 * tiles: parity 0, parity 1
    unsigned* active;  // kBatch
    unsigned tiles;
    int tilesX, tilesY, tilesZ;
    int nx, ny, nz;
};

inline size_t place(PlArgs& a, const int32_t size[3], void* scratch) {
    a.nx = size[0];
    a.ny = size[1];
    a.nz = size[2];
    a.tilesX = (a.nx + kTx - 1) / kTx;
    a.tilesY = (a.ny + kTy - 1) / kTy;
    a.tilesZ = (a.nz + kTz - 1) / kTz;
    a.tiles = static_cast<unsigned>(a.tilesX) * a.tilesY * a.tilesZ;
    ScratchArena s{static_cast<char*>(scratch), 0};
    a.active = s.take<unsigned>(kBatch);  // first: the memset of a batch starts at the allocation's start
    a.flags = s.take<uint8_t>(2 * static_cast<size_t>(a.tiles));
    return s.off;
}

__global__ __launch_bounds__(256) void k_pl_init(const PlArgs a, const uint8_t* __restrict__ classes,
                                                 const int* __restrict__ d2, int minD2, unsigned mask,
                                                 const int* __restrict__ seeds, int nSeeds, int radius,
                                                 unsigned* cost, unsigned* seedsUsed) {
    const int lane = threadIdx.x & 63;
    const size_t rows = static_cast<size_t>(a.ny) * a.nz;
    const size_t row = static_cast<size_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);  // z * ny + y
    if (row >= rows) return;  // whole waves leave
    const int z = static_cast<int>(row / a.ny), y = static_cast<int>(row - static_cast<size_t>(z) * a.ny);
    const size_t base = row * a.nx;
    const int r2 = radius * radius;  // radius <= 4096
    const int chunks = (a.nx + 63) >> 6;
    for (int k = 0; k < chunks; ++k) {
        const int x = 64 * k + lane;
        if (x >= a.nx) continue;
        const unsigned c = classes[base + x];
        bool in = c <= 2u && ((1u << c) & mask) != 0u;
        if (in && d2 != nullptr && minD2 > 0) in = d2[base + x] >= minD2;
        bool seed = false;
        for (int s = 0; s < nSeeds; ++s) {  // wave-uniform loads
            const int sx = seeds[3 * s], sy = seeds[3 * s + 1], sz = seeds[3 * s + 2];
            if (sx < 0 || sx >= a.nx || sy < 0 || sy >= a.ny || sz < 0 || sz >= a.nz) continue;  // outside: ignored
            const int dy = y - sy, dz = z - sz;
            if (dy * dy + dz * dz > r2) continue;  // wave-uniform: the bubble misses this row
            const unsigned sc = classes[(static_cast<size_t>(sz) * a.ny + sy) * a.nx + sx];
            if (sc == EMF_OCC_OCCUPIED) continue;  // ignored
            const int dx = x - sx;
            if (dx * dx + dy * dy + dz * dz <= r2) in = in || c != EMF_OCC_OCCUPIED;
            if (dx == 0 && dy == 0 && dz == 0) {
                seed = true;
                atomicAdd(seedsUsed, 1u);  // one lane per seed of the list
            }
        }
        cost[base + x] = seed ? 0u : (in ? kUnreached : kBlocked);
        if (!seed) continue;
        // a seed never changes, so nobody would flag for it: its own tile and the tiles that hold it in their halo
        const int tx0 = max(x - 1, 0) / kTx, tx1 = min(x + 1, a.nx - 1) / kTx, ty0 = max(y - 1, 0) / kTy,
                  ty1 = min(y + 1, a.ny - 1) / kTy, tz0 = max(z - 1, 0) / kTz, tz1 = min(z + 1, a.nz - 1) / kTz;
        for (int tz = tz0; tz <= tz1; ++tz)  // at most two per axis
            for (int ty = ty0; ty <= ty1; ++ty)
                for (int tx = tx0; tx <= tx1; ++tx) a.flags[(static_cast<unsigned>(tz) * a.tilesY + ty) * a.tilesX + tx] = 1;
    }
}

__device__ __forceinline__ int halo_index(int lx, int ly, int lz) {  // tile coordinates -1 .. kT
    return ((lz + 1) * kHy + (ly + 1)) * kHx + (lx + 1);
}

__global__ __launch_bounds__(kPlBlock) void k_pl_relax(const PlArgs a, unsigned* cost, unsigned maxCost, int parity,
                                                       int slot) {
    __shared__ unsigned lds[kHalo];
    const unsigned tile = blockIdx.x;
    uint8_t* cur = a.flags + static_cast<size_t>(parity) * a.tiles;
    uint8_t* next = a.flags + static_cast<size_t>(1 - parity) * a.tiles;
    if (cur[tile] == 0) return;  // the whole workgroup
    const int t = threadIdx.x;
    const int tileX = static_cast<int>(tile % a.tilesX), tileY = static_cast<int>(tile / a.tilesX % a.tilesY),
              tileZ = static_cast<int>(tile / (static_cast<unsigned>(a.tilesX) * a.tilesY));
    const int x0 = tileX * kTx, y0 = tileY * kTy, z0 = tileZ * kTz;
    for (int i = t; i < kHalo; i += kPlBlock) {
        const int hx = i % kHx, hy = i / kHx % kHy, hz = i / (kHx * kHy);
        const int x = x0 + hx - 1, y = y0 + hy - 1, z = z0 + hz - 1;
        const bool inside = x >= 0 && x < a.nx && y >= 0 && y < a.ny && z >= 0 && z < a.nz;
        lds[i] = inside ? cost[(static_cast<size_t>(z) * a.ny + y) * a.nx + x] : kBlocked;
    }
    __syncthreads();
    unsigned first[kPerThread], now[kPerThread];
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int v = t + kPlBlock * k;
        first[k] = now[k] = lds[halo_index(v % kTx, v / kTx % kTy, v / (kTx * kTy))];
    }
    int more = 1;
    for (int sweep = 0; sweep < kSweeps && more; ++sweep) {
        int changed = 0;
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            if (now[k] == kBlocked) continue;
            const int v = t + kPlBlock * k;
            const int centre = halo_index(v % kTx, v / kTx % kTy, v / (kTx * kTy));
            unsigned best = now[k];
#pragma unroll
            for (int j = 0; j < 27; ++j) {
                if (j == 13) continue;
                const int dx = j % 3 - 1, dy = j / 3 % 3 - 1, dz = j / 9 - 1;
                const unsigned w = 2u + static_cast<unsigned>(dx * dx + dy * dy + dz * dz);  // 3, 4, 5
                // another thread may be writing this word: either value is an upper bound of the neighbour's cost
                const unsigned n = lds[centre + (dz * kHy + dy) * kHx + dx];
                if (n < kBlocked) best = min(best, n + w);
            }
            if (best < now[k] && (maxCost == 0u || best <= maxCost)) {
                now[k] = best;
                lds[centre] = best;
                changed = 1;
            }
        }
        more = __syncthreads_or(changed);
    }
    // write back what changed; a changed voxel on the shell wakes the tiles that hold it in their halo
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        if (now[k] == first[k]) continue;
        const int v = t + kPlBlock * k;
        const int lx = v % kTx, ly = v / kTx % kTy, lz = v / (kTx * kTy);
        cost[(static_cast<size_t>(z0 + lz) * a.ny + (y0 + ly)) * a.nx + (x0 + lx)] = now[k];  // inside: it was not BLOCKED
        const int sx = lx == 0 ? -1 : (lx == kTx - 1 ? 1 : 0), sy = ly == 0 ? -1 : (ly == kTy - 1 ? 1 : 0),
                  sz = lz == 0 ? -1 : (lz == kTz - 1 ? 1 : 0);
        if (!(sx | sy | sz)) continue;
#pragma unroll
        for (int j = 1; j < 8; ++j) {  // the non-empty subsets of the sides this voxel lies on
            const int ex = (j & 1) ? sx : 0, ey = (j & 2) ? sy : 0, ez = (j & 4) ? sz : 0;
            if (((j & 1) && !sx) || ((j & 2) && !sy) || ((j & 4) && !sz)) continue;
            const int qx = tileX + ex, qy = tileY + ey, qz = tileZ + ez;
            if (qx < 0 || qx >= a.tilesX || qy < 0 || qy >= a.tilesY || qz < 0 || qz >= a.tilesZ) continue;
            next[(static_cast<unsigned>(qz) * a.tilesY + qy) * a.tilesX + qx] = 1;
        }
    }
    if (t == 0) {
        cur[tile] = 0;
        if (more) next[tile] = 1;  // still changing at the bound: again next round
        atomicAdd(a.active + slot, 1u);
    }
}

__global__ __launch_bounds__(kScanBlock) void k_pl_finish(const unsigned* __restrict__ cost, unsigned n, unsigned converged,
                                                          unsigned rounds, unsigned* counters) {
    __shared__ unsigned lds[kScanBlock / 64];
    const unsigned i = blockIdx.x * kScanBlock + threadIdx.x;
    unsigned total;
    block_exclusive_scan<kScanBlock / 64>(i < n && cost[i] < kBlocked ? 1u : 0u, total, lds);
    if (threadIdx.x == 0 && total) atomicAdd(counters + EMF_PLAN_FINITE, total);
    if (i == 0u) {
        counters[EMF_PLAN_CONVERGED] = converged;
        counters[EMF_PLAN_ROUNDS] = rounds;
    }
}

__global__ __launch_bounds__(256) void k_pl_paths(const unsigned* __restrict__ cost, int nx, int ny, int nz,
                                                  const int* __restrict__ goals, int nGoals, int capacity,
                                                  int* __restrict__ paths, int* __restrict__ lengths,
                                                  unsigned* __restrict__ goalCost) {
    const int lane = threadIdx.x & 63;
    const int g = static_cast<int>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (g >= nGoals) return;  // whole waves leave
    int x = goals[3 * g], y = goals[3 * g + 1], z = goals[3 * g + 2];
    const bool inside = x >= 0 && x < nx && y >= 0 && y < ny && z >= 0 && z < nz;
    const int plane = nx * ny;
    const unsigned c0 = inside ? cost[z * plane + y * nx + x] : kBlocked;
    if (lane == 0) goalCost[g] = c0;
    if (c0 >= kBlocked) {
        if (lane == 0) lengths[g] = 0;
        return;
    }
    int* out = paths + static_cast<size_t>(g) * capacity;
    const int j = lane < 13 ? lane : lane + 1;  // the 26 neighbours in ascending linear-index order
    const int dx = j % 3 - 1, dy = j / 3 % 3 - 1, dz = j / 9 - 1;
    const unsigned w = 2u + static_cast<unsigned>(dx * dx + dy * dy + dz * dz);
    const int bound = max(capacity, static_cast<int>(c0 / 3u) + 1);
    unsigned c = c0;
    int steps = 0;
    if (lane == 0 && capacity > 0) out[0] = z * plane + y * nx + x;
    for (; steps < bound && c != 0u; ++steps) {  // every step lowers the cost by at least 3
        const int qx = x + dx, qy = y + dy, qz = z + dz;
        bool hit = false;
        if (lane < 26 && qx >= 0 && qx < nx && qy >= 0 && qy < ny && qz >= 0 && qz < nz) {
            const unsigned n = cost[qz * plane + qy * nx + qx];
            hit = n < kBlocked && n + w == c;
        }
        const unsigned long long hits = __ballot(hit);
        if (hits == 0ull) break;  // only a field that did not converge
        const int step = __ffsll(static_cast<long long>(hits)) - 1;
        const int sj = step < 13 ? step : step + 1;
        const int ddx = sj % 3 - 1, ddy = sj / 3 % 3 - 1, ddz = sj / 9 - 1;
        x += ddx;
        y += ddy;
        z += ddz;
        c -= 2u + static_cast<unsigned>(ddx * ddx + ddy * ddy + ddz * ddz);
        if (lane == 0 && steps + 1 < capacity) out[steps + 1] = z * plane + y * nx + x;
    }
    if (lane == 0) lengths[g] = c == 0u ? steps + 1 : -steps;
}

int check_size(const int32_t size[3], const char* what) {
    if (!size) return fail(EMF_E_ARG, "%s: size is NULL", what);
    for (int i = 0; i < 3; ++i) {
        if (size[i] < 1) return fail(EMF_E_ARG, "%s: box axis %d has %d voxels", what, i, size[i]);
        if (size[i] > EMF_DF_MAX_AXIS)
            return fail(EMF_E_LIMIT, "%s: box axis %d has %d voxels, above %d", what, i, size[i], EMF_DF_MAX_AXIS);
    }
    const unsigned long long voxels = static_cast<unsigned long long>(size[0]) * size[1] * static_cast<unsigned long long>(size[2]);
    if (voxels > kMaxVoxels) return fail(EMF_E_LIMIT, "%s: a box of %llu voxels, above 2^29", what, voxels);
    return EMF_OK;
}

int hip_status(hipError_t e, const char* what, const char* step) {
    if (e == hipSuccess) return EMF_OK;
    (void)hipGetLastError();
    set_error("%s: %s: %s", what, step, hipGetErrorString(e));
    return static_cast<int>(e);
}

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

size_t emf_hip_planScratchBytes(const int32_t size[3]) {
    if (!size) return 0;
    for (int i = 0; i < 3; ++i)
        if (size[i] < 1 || size[i] > EMF_DF_MAX_AXIS) return 0;
    if (static_cast<unsigned long long>(size[0]) * size[1] * static_cast<unsigned long long>(size[2]) > kMaxVoxels) return 0;
    PlArgs a;
    char origin[16];
    (void)origin;
    return place(a, size, origin);  // only the offsets are used
}

int emf_hip_planCost(const uint8_t* classes, const int32_t size[3], const int32_t* d2, int32_t min_d2, uint32_t traverse_mask,
                     const int32_t* seeds, int32_t n_seeds, int32_t seed_radius, uint32_t max_cost, int32_t max_rounds,
                     uint32_t* cost, void* scratch_dev, uint32_t* counters, emf_stream_t stream) {
    EMF_TRY(check_size(size, "planCost"));  // first: the limits hold whatever the buffers are
    if (n_seeds < 1) return fail(EMF_E_ARG, "planCost: %d seeds", n_seeds);
    if (seed_radius < 0 || seed_radius > 4096) return fail(EMF_E_ARG, "planCost: a seed radius of %d voxels", seed_radius);
    if (max_cost >= kBlocked) return fail(EMF_E_ARG, "planCost: max_cost %u is no cost", max_cost);
    if (!classes || !seeds || !cost || !scratch_dev || !counters)
        return fail(EMF_E_ARG, "planCost: classes, seeds, cost, scratch or counters is NULL");
    if ((reinterpret_cast<uintptr_t>(cost) | reinterpret_cast<uintptr_t>(d2) | reinterpret_cast<uintptr_t>(counters) |
         reinterpret_cast<uintptr_t>(seeds)) & 3u ||
        (reinterpret_cast<uintptr_t>(scratch_dev) & 15u))
        return fail(EMF_E_ARG, "planCost: misaligned arrays");
    PlArgs a;
    const size_t scratchBytes = place(a, size, scratch_dev);
    const size_t rows = static_cast<size_t>(a.ny) * a.nz;
    const unsigned n = static_cast<unsigned>(rows * a.nx);
    const long long limit = max_rounds <= 0 ? static_cast<long long>(n) + 1 : static_cast<long long>(max_rounds);
    const hipStream_t s = as_stream(stream);
    EMF_TRY(hip_status(hipMemsetAsync(scratch_dev, 0, scratchBytes, s), "planCost", "memset"));
    EMF_TRY(hip_status(hipMemsetAsync(counters, 0, 4 * sizeof(uint32_t), s), "planCost", "memset"));
    hipLaunchKernelGGL(k_pl_init, dim3(ceil_div(rows, 4)), dim3(256), 0, s, a, classes, d2, min_d2, traverse_mask & 7u, seeds,
                       n_seeds, seed_radius, cost, counters + EMF_PLAN_SEEDS);
    EMF_TRY(launch_status("planCost"));
    long long rounds = 0;
    unsigned converged = 0u;
    while (!converged && rounds < limit) {
        const int batch = static_cast<int>(limit - rounds < kBatch ? limit - rounds : kBatch);
        if (rounds) EMF_TRY(hip_status(hipMemsetAsync(a.active, 0, sizeof(unsigned) * kBatch, s), "planCost", "memset"));
        for (int r = 0; r < batch; ++r)
            hipLaunchKernelGGL(k_pl_relax, dim3(a.tiles), dim3(kPlBlock), 0, s, a, cost, max_cost,
                               static_cast<int>((rounds + r) & 1), r);
        EMF_TRY(launch_status("planCost"));
        unsigned active[kBatch];
        EMF_TRY(hip_status(hipMemcpyAsync(active, a.active, sizeof(unsigned) * batch, hipMemcpyDeviceToHost, s), "planCost", "copy"));
        EMF_TRY(hip_status(hipStreamSynchronize(s), "planCost", "wait"));
        rounds += batch;
        for (int r = 0; r < batch; ++r)
            if (active[r] == 0u) converged = 1u;  // nothing was flagged: every later round of the batch was empty too
    }
    hipLaunchKernelGGL(k_pl_finish, dim3(ceil_div(n, kScanBlock)), dim3(kScanBlock), 0, s, cost, n, converged,
                       static_cast<unsigned>(rounds < 0xffffffffll ? rounds : 0xffffffffll), counters);
    return launch_status("planCost");
}

int emf_hip_planPaths(const uint32_t* cost, const int32_t size[3], const int32_t* goals, int32_t n_goals, int32_t capacity,
                      int32_t* paths, int32_t* lengths, uint32_t* goal_cost, emf_stream_t stream) {
    EMF_TRY(check_size(size, "planPaths"));
    if (n_goals < 0) return fail(EMF_E_ARG, "planPaths: %d goals", n_goals);
    if (capacity < 0) return fail(EMF_E_ARG, "planPaths: capacity %d", capacity);
    if (n_goals == 0) return EMF_OK;
    if (static_cast<unsigned long long>(n_goals) * static_cast<unsigned long long>(capacity) > 0x7fffffffull)
        return fail(EMF_E_LIMIT, "planPaths: %d goals of %d entries", n_goals, capacity);
    if (!cost || !goals || !lengths || !goal_cost || (capacity > 0 && !paths))
        return fail(EMF_E_ARG, "planPaths: cost, goals, paths, lengths or goal_cost is NULL");
    if ((reinterpret_cast<uintptr_t>(cost) | reinterpret_cast<uintptr_t>(goals) | reinterpret_cast<uintptr_t>(paths) |
         reinterpret_cast<uintptr_t>(lengths) | reinterpret_cast<uintptr_t>(goal_cost)) & 3u)
        return fail(EMF_E_ARG, "planPaths: misaligned arrays");
    hipLaunchKernelGGL(k_pl_paths, dim3(ceil_div(static_cast<size_t>(n_goals), 4)), dim3(256), 0, as_stream(stream), cost, size[0],
                       size[1], size[2], goals, n_goals, capacity, paths, lengths, goal_cost);
    return launch_status("planPaths");
}

}  // extern "C"
