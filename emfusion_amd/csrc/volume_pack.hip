// volume_pack.hip -- lossless packing of a device buffer by 1 KiB chunk (include/emf_hip.h "Packed buffers",
// DESIGN.md 5.11).
//
// A volume that a session has seen little of is mostly one word repeated: tsdf and weights start as zeros, a
// saturated weight is 64.0f everywhere behind the surface, the fg/bg counts of an object are zero outside its
// silhouette.  The packer looks at BITS only (-0.0f, NaN patterns and denormals are words like any other), in
// chunks of 256 words:
//   class 0  every word 0            -> nothing stored
//   class 1  one non-zero word       -> that word
//   class 2  anything else           -> the 1024 bytes
// The last chunk may be ragged (nbytes is a multiple of 4, not of 1024): only its valid words are read, compared
// and, on the way back, written.
//   k_pack_classify  one wave per chunk, one 16-byte load per lane; the decision is a ballot against the chunk's
//                    first word; lane 0 writes the class byte and the word
//   k_pack_sums      (uniform, literal) counts per workgroup of 256 chunks, both in one u64 (low / high half)
//   k_pack_scan      one workgroup: exclusive scan of the sums in place, the totals behind them (wave_ops.hpp)
//   k_pack_place     rank[i] = chunks of i's class before i; uniform[rank] = the word, literalChunks[rank] = i.
//                    Placement is by scan, not by atomics: the order is chunk order on every run
//   k_pack_gather    one wave per literal of a rank range: chunk literalChunks[first + w] -> arena + 1024 w
//   k_unpack_fill    one wave per chunk: zeros or the uniform word (literal chunks are left alone)
//   k_unpack_copy    one wave per literal of a rank range: arena + 1024 w -> chunk literalChunks[first + w]
// Every byte offset is 64-bit (the 1024^3 tsdf is exactly 4 GiB); chunk indices and ranks fit 32 bits by the
// entry's limit of 2^40 bytes.  A pure HBM stream: classify reads each byte once, gather re-reads the literals.
#include "common.hpp"
#include "wave_ops.hpp"

namespace emf_hip {
namespace {

constexpr int kPackBlock = 256;                 // 4 waves: 4 chunks per workgroup in the wave-per-chunk kernels
constexpr int kWavesPerBlock = kPackBlock / 64;
constexpr unsigned kChunkBytes = 1024, kChunkWords = 256;
constexpr unsigned long long kMaxBytes = 1ull << 40;

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

inline unsigned chunks_of(unsigned long long nbytes) {
    return static_cast<unsigned>((nbytes + kChunkBytes - 1) / kChunkBytes);
}

// valid words of chunk c of a buffer of nbytes (1 .. 256)
__device__ __forceinline__ unsigned valid_words(unsigned long long nbytes, unsigned c) {
    const unsigned long long left = (nbytes - static_cast<unsigned long long>(c) * kChunkBytes) >> 2;
    return left < kChunkWords ? static_cast<unsigned>(left) : kChunkWords;
}

// this lane's four words of a chunk; words at or past nvalid read as `pad` and are never touched in memory
__device__ __forceinline__ u32x4 load_lane(const unsigned* chunk, unsigned lane, unsigned nvalid, unsigned pad) {
    const unsigned w = 4u * lane;
    if (w + 4u <= nvalid) return *reinterpret_cast<const u32x4*>(chunk + w);
    u32x4 v = {pad, pad, pad, pad};
    if (w + 0u < nvalid) v.x = chunk[w + 0u];
    if (w + 1u < nvalid) v.y = chunk[w + 1u];
    if (w + 2u < nvalid) v.z = chunk[w + 2u];
    return v;
}

__device__ __forceinline__ void store_lane(unsigned* chunk, unsigned lane, unsigned nvalid, const u32x4 v) {
    const unsigned w = 4u * lane;
    if (w + 4u <= nvalid) {
        *reinterpret_cast<u32x4*>(chunk + w) = v;
        return;
    }
    if (w + 0u < nvalid) chunk[w + 0u] = v.x;
    if (w + 1u < nvalid) chunk[w + 1u] = v.y;
    if (w + 2u < nvalid) chunk[w + 2u] = v.z;
}

__device__ __forceinline__ const unsigned* chunk_at(const void* base, unsigned c) {
    return reinterpret_cast<const unsigned*>(static_cast<const char*>(base) + static_cast<unsigned long long>(c) * kChunkBytes);
}
__device__ __forceinline__ unsigned* chunk_at(void* base, unsigned c) {
    return reinterpret_cast<unsigned*>(static_cast<char*>(base) + static_cast<unsigned long long>(c) * kChunkBytes);
}

__global__ __launch_bounds__(kPackBlock) void k_pack_classify(const void* src, unsigned long long nbytes,
                                                              unsigned nchunks, uint8_t* cls, unsigned* words) {
    const unsigned c = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (c >= nchunks) return;  // (wave-uniform)
    const unsigned* chunk = chunk_at(src, c);
    const unsigned nvalid = valid_words(nbytes, c);
    const u32x4 v = load_lane(chunk, lane, nvalid, 0u);
    const unsigned first = __builtin_amdgcn_readfirstlane(v.x);  // lane 0's first word: word 0 is always valid
    const unsigned w = 4u * lane;
    const bool differs = (w + 0u < nvalid && v.x != first) || (w + 1u < nvalid && v.y != first) ||
                         (w + 2u < nvalid && v.z != first) || (w + 3u < nvalid && v.w != first);
    const bool uniform = __ballot(differs) == 0ull;
    if (lane == 0) {
        cls[c] = uniform ? (first == 0u ? 0 : 1) : 2;
        words[c] = first;
    }
}

// (uniform ? 1 : 0) | (literal ? 1 : 0) << 32
__device__ __forceinline__ unsigned long long class_count(const uint8_t* cls, unsigned i, unsigned nchunks) {
    if (i >= nchunks) return 0ull;
    const unsigned c = cls[i];
    return c == 1u ? 1ull : (c == 2u ? (1ull << 32) : 0ull);
}

__global__ __launch_bounds__(kPackBlock) void k_pack_sums(const uint8_t* cls, unsigned nchunks, unsigned long long* sums) {
    __shared__ unsigned long long lds[kWavesPerBlock];
    unsigned long long total;
    block_exclusive_scan<kWavesPerBlock>(class_count(cls, blockIdx.x * kPackBlock + threadIdx.x, nchunks), total, lds);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums[b] := sum of sums[0 .. b), sums[nblocks] := the total, totals = {uniform, literal}
__global__ __launch_bounds__(kSumsBlock) void k_pack_scan(unsigned long long* sums, unsigned nblocks, unsigned* totals) {
    __shared__ unsigned long long lds[kSumsBlock / 64];
    const unsigned long long carry = scan_sums(sums, 0u, nblocks, lds);
    if (threadIdx.x == 0) {
        sums[nblocks] = carry;
        totals[0] = static_cast<unsigned>(carry);
        totals[1] = static_cast<unsigned>(carry >> 32);
    }
}

__global__ __launch_bounds__(kPackBlock) void k_pack_place(const uint8_t* cls, const unsigned* words, unsigned nchunks,
                                                           const unsigned long long* sums, unsigned* ranks,
                                                           unsigned* uniform, unsigned* literalChunks) {
    __shared__ unsigned long long lds[kWavesPerBlock];
    const unsigned i = blockIdx.x * kPackBlock + threadIdx.x;
    unsigned long long total;
    const unsigned long long at = sums[blockIdx.x] + block_exclusive_scan<kWavesPerBlock>(class_count(cls, i, nchunks), total, lds);
    if (i >= nchunks) return;
    const unsigned c = cls[i];
    // ranks stay below the class's total, which is at most nchunks: every array here has nchunks entries
    if (c == 1u) {
        const unsigned r = static_cast<unsigned>(at);
        ranks[i] = r;
        if (uniform) uniform[r] = words[i];
    } else if (c == 2u) {
        const unsigned r = static_cast<unsigned>(at >> 32);
        ranks[i] = r;
        literalChunks[r] = i;
    } else {
        ranks[i] = 0u;
    }
}

__global__ __launch_bounds__(kPackBlock) void k_pack_gather(const void* src, unsigned long long nbytes, unsigned nchunks,
                                                            const unsigned* literalChunks, unsigned first, unsigned count,
                                                            void* arena) {
    const unsigned w = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (w >= count) return;
    const unsigned c = literalChunks[first + w];
    if (c >= nchunks) return;  // (not something k_pack_place writes: stay inside the source whatever the list holds)
    const u32x4 v = load_lane(chunk_at(src, c), lane, valid_words(nbytes, c), 0u);  // a ragged tail is zero-padded
    store_lane(chunk_at(arena, w), lane, kChunkWords, v);
}

__global__ __launch_bounds__(kPackBlock) void k_unpack_fill(void* dst, unsigned long long nbytes, unsigned nchunks,
                                                            const uint8_t* cls, const unsigned* ranks,
                                                            const unsigned* uniform, unsigned nuniform) {
    const unsigned c = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (c >= nchunks) return;
    const unsigned k = cls[c];
    if (k > 1u) return;  // literals: k_unpack_copy
    unsigned word = 0u;
    if (k == 1u) {
        const unsigned r = ranks[c];
        if (r >= nuniform) return;  // (ranks of another class array: write nothing rather than read past the words)
        word = uniform[r];
    }
    const u32x4 v = {word, word, word, word};
    store_lane(chunk_at(dst, c), lane, valid_words(nbytes, c), v);
}

__global__ __launch_bounds__(kPackBlock) void k_unpack_copy(void* dst, unsigned long long nbytes, unsigned nchunks,
                                                            const unsigned* literalChunks, unsigned first, unsigned count,
                                                            const void* arena) {
    const unsigned w = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (w >= count) return;
    const unsigned c = literalChunks[first + w];
    if (c >= nchunks) return;
    const u32x4 v = load_lane(chunk_at(arena, w), lane, kChunkWords, 0u);
    store_lane(chunk_at(dst, c), lane, valid_words(nbytes, c), v);
}

int check_buffer(const void* p, uint64_t nbytes, const char* what, const char* name) {
    if (p == nullptr) return fail(EMF_E_NULL, "%s: %s is NULL", what, name);
    if (nbytes == 0 || (nbytes & 3u) != 0) return fail(EMF_E_ARG, "%s: %llu bytes (a positive multiple of 4)", what, (unsigned long long)nbytes);
    if (nbytes > kMaxBytes) return fail(EMF_E_LIMIT, "%s: %llu bytes (at most 2^40)", what, (unsigned long long)nbytes);
    if ((reinterpret_cast<uintptr_t>(p) & 15u) != 0) return fail(EMF_E_ARG, "%s: %s is not 16-byte aligned", what, name);
    return EMF_OK;
}

// a rank range inside the nchunks entries of the chunk list
int check_range(uint32_t first, uint32_t count, unsigned nchunks, const char* what) {
    if (first > nchunks || count > nchunks - first)
        return fail(EMF_E_ARG, "%s: literal ranks [%u, %u + %u) of a buffer of %u chunks", what, first, first, count, nchunks);
    return EMF_OK;
}

inline dim3 wave_grid(unsigned waves) { return dim3(ceil_div(waves, kWavesPerBlock)); }

}  // namespace
}  // namespace emf_hip

using namespace emf_hip;

extern "C" {

size_t emf_hip_packScratchBytes(uint64_t nbytes) {
    if (nbytes == 0 || nbytes > kMaxBytes) return 0;
    return sizeof(unsigned long long) * (static_cast<size_t>(ceil_div(chunks_of(nbytes), kPackBlock)) + 1);
}

int emf_hip_packClassify(const void* src, uint64_t nbytes, uint8_t* classes, uint32_t* words, emf_stream_t stream) {
    EMF_TRY(check_buffer(src, nbytes, "packClassify", "src"));
    EMF_REQUIRE_PTR(classes);
    EMF_REQUIRE_PTR(words);
    const unsigned nchunks = chunks_of(nbytes);
    hipLaunchKernelGGL(k_pack_classify, wave_grid(nchunks), dim3(kPackBlock), 0, as_stream(stream), src,
                       static_cast<unsigned long long>(nbytes), nchunks, classes, words);
    return launch_status("packClassify");
}

int emf_hip_packRank(const uint8_t* classes, const uint32_t* words, uint64_t nbytes, void* scratch_dev, uint32_t* ranks,
                     uint32_t* uniform, uint32_t* literal_chunks, uint32_t* totals, emf_stream_t stream) {
    if (nbytes == 0 || nbytes > kMaxBytes) return fail(EMF_E_LIMIT, "packRank: %llu bytes (1 .. 2^40)", (unsigned long long)nbytes);
    EMF_REQUIRE_PTR(classes);
    EMF_REQUIRE_PTR(scratch_dev);
    EMF_REQUIRE_PTR(ranks);
    EMF_REQUIRE_PTR(literal_chunks);
    EMF_REQUIRE_PTR(totals);
    if ((words == nullptr) != (uniform == nullptr)) return fail(EMF_E_NULL, "packRank: words and uniform go together");
    if ((reinterpret_cast<uintptr_t>(scratch_dev) & 7u) != 0) return fail(EMF_E_ARG, "packRank: scratch_dev is not 8-byte aligned");
    const unsigned nchunks = chunks_of(nbytes), nblocks = ceil_div(nchunks, kPackBlock);
    unsigned long long* sums = static_cast<unsigned long long*>(scratch_dev);
    hipLaunchKernelGGL(k_pack_sums, dim3(nblocks), dim3(kPackBlock), 0, as_stream(stream), classes, nchunks, sums);
    hipLaunchKernelGGL(k_pack_scan, dim3(1), dim3(kSumsBlock), 0, as_stream(stream), sums, nblocks, totals);
    hipLaunchKernelGGL(k_pack_place, dim3(nblocks), dim3(kPackBlock), 0, as_stream(stream), classes, words, nchunks,
                       static_cast<const unsigned long long*>(sums), ranks, uniform, literal_chunks);
    return launch_status("packRank");
}

int emf_hip_packGather(const void* src, uint64_t nbytes, const uint32_t* literal_chunks, uint32_t first, uint32_t count,
                       void* arena, emf_stream_t stream) {
    EMF_TRY(check_buffer(src, nbytes, "packGather", "src"));
    const unsigned nchunks = chunks_of(nbytes);
    EMF_TRY(check_range(first, count, nchunks, "packGather"));
    if (count == 0) return EMF_OK;
    EMF_REQUIRE_PTR(literal_chunks);
    EMF_TRY(check_buffer(arena, static_cast<uint64_t>(count) * kChunkBytes, "packGather", "arena"));
    hipLaunchKernelGGL(k_pack_gather, wave_grid(count), dim3(kPackBlock), 0, as_stream(stream), src,
                       static_cast<unsigned long long>(nbytes), nchunks, literal_chunks, first, count, arena);
    return launch_status("packGather");
}

int emf_hip_unpackFill(void* dst, uint64_t nbytes, const uint8_t* classes, const uint32_t* ranks, const uint32_t* uniform,
                       uint32_t nuniform, emf_stream_t stream) {
    EMF_TRY(check_buffer(dst, nbytes, "unpackFill", "dst"));
    EMF_REQUIRE_PTR(classes);
    EMF_REQUIRE_PTR(ranks);
    const unsigned nchunks = chunks_of(nbytes);
    if (nuniform > nchunks) return fail(EMF_E_ARG, "unpackFill: %u uniform words for %u chunks", nuniform, nchunks);
    if (nuniform) EMF_REQUIRE_PTR(uniform);
    hipLaunchKernelGGL(k_unpack_fill, wave_grid(nchunks), dim3(kPackBlock), 0, as_stream(stream), dst,
                       static_cast<unsigned long long>(nbytes), nchunks, classes, ranks, uniform, nuniform);
    return launch_status("unpackFill");
}

int emf_hip_unpackLiterals(void* dst, uint64_t nbytes, const uint32_t* literal_chunks, uint32_t first, uint32_t count,
                           const void* arena, emf_stream_t stream) {
    EMF_TRY(check_buffer(dst, nbytes, "unpackLiterals", "dst"));
    const unsigned nchunks = chunks_of(nbytes);
    EMF_TRY(check_range(first, count, nchunks, "unpackLiterals"));
    if (count == 0) return EMF_OK;
    EMF_REQUIRE_PTR(literal_chunks);
    EMF_TRY(check_buffer(arena, static_cast<uint64_t>(count) * kChunkBytes, "unpackLiterals", "arena"));
    hipLaunchKernelGGL(k_unpack_copy, wave_grid(count), dim3(kPackBlock), 0, as_stream(stream), dst,
                       static_cast<unsigned long long>(nbytes), nchunks, literal_chunks, first, count, arena);
    return launch_status("unpackLiterals");
}

}  // extern "C"
