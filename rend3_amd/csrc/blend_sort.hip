// blend_sort.hip -- Sorting::BLENDING on the device: the back-to-front order of the blend-key objects and the exclusive scan of
// their triangle counts, the two buffers k_blend_setup (kernels_raster.h) reads.  Contract and terms: blend_sort.h.
//
// The sort key is host.blend_sort_key (rend3_amd/host.py), bit for bit: -dist as an order-preserving u32.  The unit is built with
// -ffp-contract=off, so (dx * dx + dy * dy) + dz * dz rounds after every operation as glam's distance_squared does.
//
// Small path (n <= R3N_BLEND_SORT_SMALL): k_blend_sort_small, one workgroup of 1024 threads.  The 64-bit values (key << 32 | i), i
// the position in the slot-ascending set, are unique, so the bitonic network in LDS gives the one possible answer.
// Large path: stable LSD radix sort of (key, i), four passes of 8 bits.  A pass is a digit histogram per tile (k_bs_hist), one
// exclusive scan of the digit-major table (k_bs_scan) and a scatter that keeps the order of equal digits (k_bs_scatter); the
// input is slot-ascending, so stable on the key IS the (key, slot) order.  Equal digits inside a wave are ranked with ballots
// (match8): one LDS update per digit group, no per-lane atomics.  Then k_bs_gather / k_bs_scan / k_bs_rank form the rank scan.
// Wave64 throughout; every grid depends on n alone.
#include <hip/hip_runtime.h>

#include "blend_sort.h"
#include "device_math.h"

namespace {

#define BS_NTRI_MASK 0x3FFFFFFFu  // == R3N_META_NTRI_MASK (kernels_cull.h; r3n.hip asserts the two agree)
#define BS_ITEMS (R3N_BLEND_SORT_TILE / 256u)  // keys per thread of a 256-thread tile kernel

// f32 -> u32 with the same order: a negative float's bits grow with its magnitude, so they are inverted; a positive one gets the
// sign bit set.  dist is never negative (a sum of squares) and never -0.0, so key = -dist is never +0.0: the one pair of equal
// floats this mapping would tell apart (-0.0 -> 0x7FFFFFFF, +0.0 -> 0x80000000) cannot meet.  -inf (dist = +inf) -> 0x007FFFFF.
R3N_DEV uint32_t blend_sort_key(const float cam[3], const float *__restrict__ loc) {
    const float dx = cam[0] - loc[0], dy = cam[1] - loc[1], dz = cam[2] - loc[2];
    const float dist = (dx * dx + dy * dy) + dz * dz;
    const uint32_t b = __float_as_uint(-dist);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// exclusive scan of one value per thread over a workgroup of NW waves; `total` = the sum of all.  `ws` holds NW words.
template <uint32_t NW>
R3N_DEV uint32_t block_exclusive_scan(uint32_t v, uint32_t *ws, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    if (lane == 63u) ws[w] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t k = 0; k < NW; ++k) {
        const uint32_t t = ws[k];
        if (k < w) before += t;
        all += t;
    }
    __syncthreads();  // ws is free again
    total = all;
    return before + inc - v;
}

// rank_base[first + j] for j in [0, count): in: the triangle counts, out: carry + their exclusive scan.  Returns carry + their sum.
// Rounds of one coalesced word per thread; count and carry are uniform over the workgroup.
template <uint32_t NT>
R3N_DEV uint32_t scan_rounds(uint32_t *__restrict__ rank_base, uint32_t first, uint32_t count, uint32_t carry, uint32_t *ws) {
    for (uint32_t r = 0; r < count; r += NT) {
        const uint32_t j = r + threadIdx.x;
        const uint32_t t = j < count ? rank_base[first + j] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan<NT / 64u>(t, ws, total);
        if (j < count) rank_base[first + j] = carry + ex;
        carry += total;
    }
    return carry;
}

// ------------------------------------------------------------------------------------------------ small path
// m: the power of two >= n the network sorts (padding sorts last: no key has the top bit set AND all others, see blend_sort_key)
__global__ __launch_bounds__(1024) void k_blend_sort_small(BlendSortArgs a, uint32_t m) {
    __shared__ unsigned long long kv[R3N_BLEND_SORT_SMALL];
    __shared__ uint32_t ws[16];
    const uint32_t tid = threadIdx.x, n = a.n;
    for (uint32_t i = tid; i < m; i += 1024u)
        kv[i] = i < n ? ((unsigned long long)blend_sort_key(a.camera, a.locations + 3u * (size_t)i) << 32) | i : ~0ull;
    __syncthreads();
    for (uint32_t k = 2; k <= m; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < (m >> 1); t += 1024u) {
                const uint32_t lo = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), hi = lo | j;
                const unsigned long long x = kv[lo], y = kv[hi];
                if ((x > y) == ((lo & k) == 0u)) { kv[lo] = y; kv[hi] = x; }
            }
            __syncthreads();
        }
    for (uint32_t j = tid; j < n; j += 1024u) {
        const uint32_t slot = a.slots[(uint32_t)kv[j]];
        a.order[j] = slot;
        a.rank_base[j] = a.obj_meta[slot] & BS_NTRI_MASK;
    }
    __syncthreads();  // scan_rounds reads what other threads of this workgroup wrote to global memory
    const uint32_t total = scan_rounds<1024u>(a.rank_base, 0u, n, 0u, ws);
    if (tid == 0u) a.rank_base[n] = total;
}

// ------------------------------------------------------------------------------------------------ large path
__global__ __launch_bounds__(256) void k_bs_keys(BlendSortArgs a, uint32_t *__restrict__ keys) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < a.n) keys[i] = blend_sort_key(a.camera, a.locations + 3u * (size_t)i);
}

// the lanes of this wave that hold the same 8-bit digit as this one (lanes with !valid: none, and they are in no mask)
R3N_DEV unsigned long long match8(uint32_t d, bool valid) {
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (uint32_t b = 0; b < 8u; ++b) {
        const bool bit = ((d >> b) & 1u) != 0u;
        const unsigned long long s = __ballot(bit);
        m &= bit ? s : ~s;
    }
    return valid ? m : 0ull;
}

// A tile is R3N_BLEND_SORT_TILE consecutive keys; wave w of the workgroup owns the w-th quarter of it and walks it 64 keys a round,
// so "earlier in the tile" is (wave, round, lane) -- the order k_bs_scatter keeps.
R3N_DEV uint32_t tile_element(uint32_t r) {
    return blockIdx.x * R3N_BLEND_SORT_TILE + (threadIdx.x >> 6) * (64u * BS_ITEMS) + r * 64u + (threadIdx.x & 63u);
}

// hist[d * tiles + tile] = keys of the tile whose digit is d
__global__ __launch_bounds__(256) void k_bs_hist(const uint32_t *__restrict__ keys, uint32_t n, uint32_t shift, uint32_t *__restrict__ hist) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll 4
    for (uint32_t r = 0; r < BS_ITEMS; ++r) {
        const uint32_t e = tile_element(r);
        const bool valid = e < n;
        const uint32_t d = valid ? (keys[e] >> shift) & 255u : 0u;
        const unsigned long long same = match8(d, valid);
        if (valid && (same & ((1ull << lane) - 1ull)) == 0ull) atomicAdd(&h[d], (uint32_t)__popcll(same));  // one add per digit group
    }
    __syncthreads();
    hist[threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

// in-place exclusive scan of m words, one workgroup
__global__ __launch_bounds__(1024) void k_bs_scan(uint32_t *__restrict__ data, uint32_t m) {
    __shared__ uint32_t ws[16];
    const uint32_t per = (m + 1023u) / 1024u;
    const uint32_t lo = min(threadIdx.x * per, m), hi = min(lo + per, m);
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += data[i];
    uint32_t total;
    uint32_t run = block_exclusive_scan<16u>(sum, ws, total);
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t t = data[i];
        data[i] = run;
        run += t;
    }
}

// `offsets`: the scanned histogram table.  idx_in == nullptr: the payload is the element's own position (first pass).
__global__ __launch_bounds__(256) void k_bs_scatter(const uint32_t *__restrict__ keys_in, const uint32_t *__restrict__ idx_in,
                                                    uint32_t *__restrict__ keys_out, uint32_t *__restrict__ idx_out, uint32_t n,
                                                    uint32_t shift, const uint32_t *__restrict__ offsets) {
    __shared__ uint32_t cnt[4][256];  // per wave and digit: keys seen so far; then the keys of the earlier waves
    __shared__ uint32_t goff[256];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) cnt[k][threadIdx.x] = 0u;
    goff[threadIdx.x] = offsets[threadIdx.x * gridDim.x + blockIdx.x];
    __syncthreads();
    uint32_t key[BS_ITEMS], val[BS_ITEMS], rank[BS_ITEMS];
#pragma unroll
    for (uint32_t r = 0; r < BS_ITEMS; ++r) {
        const uint32_t e = tile_element(r);
        const bool valid = e < n;
        key[r] = valid ? keys_in[e] : 0u;
        val[r] = valid ? (idx_in ? idx_in[e] : e) : 0u;
        const uint32_t d = (key[r] >> shift) & 255u;
        const unsigned long long same = match8(d, valid);
        const uint32_t lower = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        const uint32_t seen = valid ? cnt[w][d] : 0u;  // the whole digit group reads the count ...
        __builtin_amdgcn_wave_barrier();
        if (valid && lower == 0u) cnt[w][d] = seen + (uint32_t)__popcll(same);  // ... before its first lane advances it
        __builtin_amdgcn_wave_barrier();
        rank[r] = seen + lower;
    }
    __syncthreads();
    {
        uint32_t run = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t t = cnt[k][threadIdx.x];
            cnt[k][threadIdx.x] = run;
            run += t;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < BS_ITEMS; ++r) {
        if (tile_element(r) >= n) continue;
        const uint32_t d = (key[r] >> shift) & 255u;
        const uint32_t pos = goff[d] + cnt[w][d] + rank[r];
        if (pos < n) {  // (always, when the table is this pass's histogram)
            keys_out[pos] = key[r];
            idx_out[pos] = val[r];
        }
    }
}

// order, the unscanned triangle counts (into rank_base) and their sum per tile
__global__ __launch_bounds__(256) void k_bs_gather(BlendSortArgs a, const uint32_t *__restrict__ idx, uint32_t *__restrict__ sums) {
    __shared__ uint32_t ws[4];
    uint32_t sum = 0;
    for (uint32_t r = 0; r < BS_ITEMS; ++r) {
        const uint32_t j = blockIdx.x * R3N_BLEND_SORT_TILE + r * 256u + threadIdx.x;
        if (j >= a.n) break;
        const uint32_t i = idx[j];
        const uint32_t slot = a.slots[i < a.n ? i : 0u];
        const uint32_t t = a.obj_meta[slot] & BS_NTRI_MASK;
        a.order[j] = slot;
        a.rank_base[j] = t;
        sum += t;
    }
    uint32_t total;
    (void)block_exclusive_scan<4u>(sum, ws, total);
    if (threadIdx.x == 0u) sums[blockIdx.x] = total;
}

// `sums`: scanned.  The last tile also writes rank_base[n], the total.
__global__ __launch_bounds__(256) void k_bs_rank(BlendSortArgs a, const uint32_t *__restrict__ sums) {
    __shared__ uint32_t ws[4];
    const uint32_t first = blockIdx.x * R3N_BLEND_SORT_TILE;
    const uint32_t count = min(R3N_BLEND_SORT_TILE, a.n - first);
    const uint32_t end = scan_rounds<256u>(a.rank_base, first, count, sums[blockIdx.x], ws);
    if (blockIdx.x == gridDim.x - 1u && threadIdx.x == 0u) a.rank_base[a.n] = end;
}

uint32_t tiles_of(uint32_t n) { return (uint32_t)(((uint64_t)n + R3N_BLEND_SORT_TILE - 1u) / R3N_BLEND_SORT_TILE); }

}  // namespace

extern "C" size_t r3n_internal_blend_sort_scratch_words(uint32_t n) {
    if (n <= R3N_BLEND_SORT_SMALL) return 0;
    // keys and payloads, twice (the passes alternate between them); the digit-major histogram table; the tile sums of the scan
    return 4u * (size_t)n + 257u * (size_t)tiles_of(n);
}

extern "C" int r3n_internal_blend_sort(const BlendSortArgs *ap, hipStream_t stream) {
    const BlendSortArgs &a = *ap;
    const uint32_t n = a.n;
    if (n == 0u) return (int)hipSuccess;
    if (n <= R3N_BLEND_SORT_SMALL) {
        uint32_t m = 1;
        while (m < n) m <<= 1;
        hipLaunchKernelGGL(k_blend_sort_small, dim3(1), dim3(1024), 0, stream, a, m);
        return (int)hipGetLastError();
    }
    const uint32_t tiles = tiles_of(n);
    uint32_t *keys[2] = {a.scratch, a.scratch + n}, *idx[2] = {a.scratch + 2u * (size_t)n, a.scratch + 3u * (size_t)n};
    uint32_t *hist = a.scratch + 4u * (size_t)n, *sums = hist + 256u * (size_t)tiles;
    hipLaunchKernelGGL(k_bs_keys, dim3((n + 255u) / 256u), dim3(256), 0, stream, a, keys[0]);
    for (uint32_t pass = 0; pass < 4u; ++pass) {
        const uint32_t in = pass & 1u, out = in ^ 1u, shift = 8u * pass;
        hipLaunchKernelGGL(k_bs_hist, dim3(tiles), dim3(256), 0, stream, keys[in], n, shift, hist);
        hipLaunchKernelGGL(k_bs_scan, dim3(1), dim3(1024), 0, stream, hist, 256u * tiles);
        hipLaunchKernelGGL(k_bs_scatter, dim3(tiles), dim3(256), 0, stream, keys[in], pass ? idx[in] : nullptr, keys[out], idx[out], n, shift, hist);
    }
    hipLaunchKernelGGL(k_bs_gather, dim3(tiles), dim3(256), 0, stream, a, idx[0], sums);  // four passes: the result is back in [0]
    hipLaunchKernelGGL(k_bs_scan, dim3(1), dim3(1024), 0, stream, sums, tiles);
    hipLaunchKernelGGL(k_bs_rank, dim3(tiles), dim3(256), 0, stream, a, sums);
    return (int)hipGetLastError();
}
