// ddstore_amd CDNA4 (gfx950) gather/pack kernels.
//
// Design notes (MI355X):
//  - These kernels are bandwidth-bound data movers, no MFMA. The store's
//    reference counterpart moved one row per blocking MPI_Get/fi_read
//    (reference: include/ddstore.hpp:229-237, src/common.cxx:332-343). Here
//    one launch moves a whole minibatch: peer shards are directly readable
//    through hipIpc-mapped pointers, so a remote row is a plain vector load
//    that the fabric routes over xGMI.
//  - 16 B/lane loads (uint4) on the fast path: 64-lane wave x 16 B = 1 KiB
//    per instruction, the gfx950 coalescing sweet spot.
//  - The owner directory (world_size+1 prefix sums, <=8 on one node) is
//    staged in LDS; owner lookup is a ~3-7 step binary search over LDS.
//    The tiled fixed-stride gather takes it in its kernel arguments instead
//    when it fits (see k_gather_tiled).
//  - Grids are grid-stride with a cap: >>256 workgroups to fill 8 XCDs,
//    capped so small launches don't pay dispatch for idle blocks. The tiled
//    gather runs a persistent grid sized from the CU count.

#include "ddstore_kernels.h"

#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp8.h>
#include <type_traits>
#include <cstdlib>
#include <string>

namespace ddstore {

namespace {

constexpr int kBlock = 256;
constexpr int64_t kMaxBlocks = 32768;   // 128 blocks/CU worth of headroom

inline int n_blocks(int64_t work_items) {
    int64_t b = (work_items + kBlock - 1) / kBlock;
    if (b < 1) b = 1;
    if (b > kMaxBlocks) b = kMaxBlocks;
    return (int)b;
}

template <typename T, int N>
struct alignas(sizeof(T) * N) VecT {
    T v[N];
};

__device__ __forceinline__ int owner_of(const int64_t* prefix, int nparts, int64_t row) {
    // prefix[0] = 0; find p with prefix[p] <= row < prefix[p+1].
    // (reference equivalent: linear `sortedsearch`, src/ddstore.cxx:5-17)
    int lo = 0, hi = nparts - 1;
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= row) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The owner directory staged in LDS, declared `__shared__` by the kernel:
// the shard base pointers (as P) and NPFX prefix-sum arrays -- prefix[0]
// counts rows (samples), and the CSR kernels add prefix[1], the element
// counts. load() is the strided copy from the device arrays plus the barrier.
template <typename P, int NPFX = 1>
struct LdsDir {
    int64_t prefix[NPFX][DDS_MAX_PARTS + 1];
    P base[DDS_MAX_PARTS];

    __device__ __forceinline__ void load(const void* const* peer_base, int nparts,
                                         const int64_t* gprefix0,
                                         const int64_t* gprefix1 = nullptr) {
        for (int i = threadIdx.x; i <= nparts; i += kBlock) {
            prefix[0][i] = gprefix0[i];
            if constexpr (NPFX == 2) prefix[1][i] = gprefix1[i];
        }
        for (int i = threadIdx.x; i < nparts; i += kBlock)
            base[i] = reinterpret_cast<P>(peer_base[i]);
        __syncthreads();
    }
};

template <typename P, int NPFX>
__device__ __forceinline__ int owner_of(const LdsDir<P, NPFX>& d, int nparts, int64_t row) {
    return owner_of(d.prefix[0], nparts, row);
}

// a bad index is skipped and counted by the caller, never read out of bounds
template <typename P, int NPFX>
__device__ __forceinline__ bool out_of_range(const LdsDir<P, NPFX>& d, int nparts,
                                             int64_t g) {
    return g < 0 || g >= d.prefix[0][nparts];
}

template <typename T>
constexpr bool is_fp8_v =
    std::is_same_v<T, __hip_fp8_e4m3> || std::is_same_v<T, __hip_fp8_e5m2>;

// f64 -> f32 as a rounding of its own. HIP compiles with -ffp-contract=fast,
// which flags every conversion `contract`; the backend then merges
// (f16)(float)x into ONE f64 -> f16 rounding (and the same for bf16), while
// the contract (docs/API.md, cast semantics) and the host backend round
// twice. With contraction off for this one conversion the merge does not
// happen.
__device__ __forceinline__ float f64_to_f32(double v) {
#pragma clang fp contract(off)
    return static_cast<float>(v);
}

template <typename Tout, typename Tin>
__device__ __forceinline__ Tout cvt(Tin v) {
    if constexpr (std::is_same_v<Tout, Tin>) {
        return v;
    } else if constexpr (std::is_same_v<Tin, double> &&
                         (std::is_same_v<Tout, __half> ||
                          std::is_same_v<Tout, __hip_bfloat16>)) {
        return cvt<Tout, float>(f64_to_f32(v));
    } else if constexpr (std::is_same_v<Tout, uint8_t> &&
                         std::is_floating_point_v<Tin>) {
        // A value outside 0..255 is unspecified by the contract, but it must
        // stay in its own byte. The plain cast is undefined there, so the
        // compiler packed the unmasked 32-bit converts of a 16-B chunk with
        // ORs and -3.0f (0xFFFFFFFD) overwrote its neighbours. Through int32
        // the narrowing is an integer truncation, which is masked; the low
        // byte is what the cast gave before, element by element.
        return static_cast<uint8_t>(static_cast<int32_t>(v));
    } else if constexpr (std::is_same_v<Tin, __half>) {
        return cvt<Tout, float>(__half2float(v));
    } else if constexpr (std::is_same_v<Tin, __hip_bfloat16>) {
        return cvt<Tout, float>(__bfloat162float(v));
    } else if constexpr (is_fp8_v<Tin>) {
        return cvt<Tout, float>(static_cast<float>(v));
    } else if constexpr (std::is_same_v<Tout, __half>) {
        return __float2half(static_cast<float>(v));
    } else if constexpr (std::is_same_v<Tout, __hip_bfloat16>) {
        return __float2bfloat16(static_cast<float>(v));
    } else if constexpr (is_fp8_v<Tout>) {
        // The fp8 constructors saturate to the largest finite value; the
        // contract (docs/API.md, cast semantics) is torch's: past the
        // midpoint above the largest finite value, ties to even deciding the
        // midpoint itself, e4m3fn gives NaN (also for +-inf) and e5m2 +-inf.
        // A NaN fails both compares and converts as before.
        const float f = static_cast<float>(v);
        Tout r(f);
        if constexpr (std::is_same_v<Tout, __hip_fp8_e4m3>) {
            if (fabsf(f) > 464.0f) r.__x = 0x7F;
        } else {
            if (fabsf(f) >= 61440.0f) r.__x = f < 0.0f ? 0xFC : 0x7C;
        }
        return r;
    } else {
        return static_cast<Tout>(v);
    }
}

// ---------------------------------------------------------------------------
// Per-element transforms of the fixed-stride gathers: byte move, dtype cast,
// and the fused affine out = cast(in) * scale + shift with float outputs only
// (data-loader normalization fused into the fetch: store u8/fp8/f16 samples,
// gather normalized f32/bf16/f16 minibatches in one pass). Math in f32.
// ---------------------------------------------------------------------------
// kNeedsCol: the transform wants the element's column (its flat position in
// the row or CSR element). Only then do the kernels form one, so the other
// instantiations keep the code they had before the column existed.
struct XfIdentity {
    static constexpr bool kNeedsCol = false;
    template <typename Tout, typename Tin>
    __device__ __forceinline__ Tout apply(Tin v) const { return v; }
};
struct XfCast {
    static constexpr bool kNeedsCol = false;
    template <typename Tout, typename Tin>
    __device__ __forceinline__ Tout apply(Tin v) const { return cvt<Tout>(v); }
};
struct XfAffine {
    static constexpr bool kNeedsCol = false;
    float scale, shift;
    // Always 0, but only the host knows. For an f16 output the compiler
    // selects v_fma_mixlo_f16 for fmaf + convert, which rounds the exact sum
    // ONCE, to f16, while the contract is the fma rounded to f32 and that
    // value cast. OR-ing the f32 result with this kernel argument keeps the
    // two roundings apart (one v_or_b32 per element, f16 outputs only).
    uint32_t opaque_zero = 0;
    template <typename Tout, typename Tin>
    __device__ __forceinline__ Tout apply(Tin v) const {
        float y = fmaf(cvt<float>(v), scale, shift);
        if constexpr (std::is_same_v<Tout, __half>)
            y = __uint_as_float(__float_as_uint(y) | opaque_zero);
        return cvt<Tout>(y);
    }
};
// Per-column affine: out = fma(cast(in), scale[col], shift[col]), the same
// contract as XfAffine with one (scale, shift) pair per column. The vectors
// hold `disp` floats each, 16-B aligned (the host checks), and are read
// through the cache, as aligned vector loads wherever a chunk lies in one row.
//
// Cache against LDS (both vectors staged once per persistent block of the
// tiled kernel), MI355X, flagship shape (262,144 x 128 f32 -> bf16, 4 rotating
// outputs and index sets): 34.7 us per fetch through the cache, 34.8 us from
// LDS, the scalar XfAffine 34.9 / 35.7 us in the same two runs -- equal within
// the spread between repetitions (0.3 to 2.8 us). The cache form has no cap
// on the row length and no barrier, so it stayed and the LDS variant was
// taken out again (profiles/colnorm_ab.txt).
struct XfAffineCol {
    static constexpr bool kNeedsCol = true;
    const float* scale;
    const float* shift;
    uint32_t opaque_zero = 0;  // see XfAffine
    template <typename Tout, typename Tin>
    __device__ __forceinline__ Tout apply(Tin v, float sc, float sh) const {
        float y = fmaf(cvt<float>(v), sc, sh);
        if constexpr (std::is_same_v<Tout, __half>)
            y = __uint_as_float(__float_as_uint(y) | opaque_zero);
        return cvt<Tout>(y);
    }
};

// One VEC-element chunk through `xf`. For a column transform, `col0` is the
// column of the chunk's first element and sc/sh the two vectors; CONTIG says that col0 is a multiple of VEC and the chunk lies inside
// one row, so the VEC scales and shifts are one aligned vector load each.
// Without CONTIG the column wraps to 0 at `disp`, element by element.
template <typename Tout, int VEC, bool CONTIG, typename Xf, typename Tin>
__device__ __forceinline__ void xf_chunk(const Xf& xf, const float* sc, const float* sh,
                                         const VecT<Tin, VEC>& vin, VecT<Tout, VEC>& vout,
                                         uint32_t col0, uint32_t disp = 0) {
    if constexpr (!Xf::kNeedsCol) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) vout.v[k] = xf.template apply<Tout>(vin.v[k]);
    } else if constexpr (CONTIG) {
        const VecT<float, VEC> s = *reinterpret_cast<const VecT<float, VEC>*>(sc + col0);
        const VecT<float, VEC> h = *reinterpret_cast<const VecT<float, VEC>*>(sh + col0);
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            vout.v[k] = xf.template apply<Tout>(vin.v[k], s.v[k], h.v[k]);
    } else {
        uint32_t cc = col0;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            vout.v[k] = xf.template apply<Tout>(vin.v[k], sc[cc], sh[cc]);
            cc = cc + 1 == disp ? 0 : cc + 1;
        }
    }
}

// ---------------------------------------------------------------------------
// One-shot fixed-stride row gather: thread t moves VEC-element chunk
// (t % chunks_per_row) of row (t / chunks_per_row) through `xf`. Consecutive
// lanes walk consecutive chunks of one row -> coalesced loads and stores; the
// per-thread i64 divide is hidden under the memory traffic. Requires
// row_elems % VEC == 0 and out aligned to VEC elements (the host checks).
//
// Cast and affine, VEC = 16 / sizeof(Tout) -- measured optimum on MI355X: the
// OUTPUT side exactly 16 B per thread, input side 16*in/out bytes (f32->bf16:
// 32B-in/16B-out = 21.2 us vs 27.4 us for 16B/8B; u8->f32: 4B-in/16B-out =
// 20.9 us vs 26.0 us for 16B/64B) -- stores are the side that cannot be split
// by the memory system, so keep them at dwordx4 (scalar bf16/f16 loads cost
// ~2-2.5x -- cdna_hip_programming.md G13). VEC = 1 is their element-wise
// fallback for rows or outputs that do not allow it.
//
// The same-dtype byte move is XfIdentity with VEC = 1 over a 16-B (uint4) or
// 32-B (VecT<uint4, 2>) element. 32 B (two dwordx4 loads in flight per
// thread) measured faster than 16 B when rows allow -- same finding as the
// cast, where 32B-read threads beat 16B-read threads on byte rate.
// ---------------------------------------------------------------------------
template <typename Tin, typename Tout, int VEC, typename Xf>
__global__ void __launch_bounds__(kBlock)
k_gather_oneshot(const void* const* peer_base, const int64_t* gprefix, int nparts,
                 const int64_t* idx, int64_t nidx, int64_t row_elems, Xf xf,
                 Tout* __restrict__ out, unsigned long long* oob) {
    using Vin = VecT<Tin, VEC>;
    using Vout = VecT<Tout, VEC>;
    __shared__ LdsDir<const Tin*> dir;
    dir.load(peer_base, nparts, gprefix);

    const int64_t cpr = row_elems / VEC;  // chunks per row
    const int64_t total = nidx * cpr;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * kBlock) {
        const int64_t r = t / cpr;
        const int64_t c = t - r * cpr;
        const int64_t g = idx[r];
        if (out_of_range(dir, nparts, g)) {  // skip instead of OOB read
            if (c == 0) atomicAdd(oob, 1ull);
            continue;
        }
        const int p = owner_of(dir, nparts, g);
        const Vin vin = *reinterpret_cast<const Vin*>(
            dir.base[p] + (g - dir.prefix[0][p]) * row_elems + c * VEC);
        Vout vout;
        if constexpr (Xf::kNeedsCol)  // a chunk never leaves its row
            xf_chunk<Tout, VEC, true>(xf, xf.scale, xf.shift, vin, vout,
                                      (uint32_t)c * VEC);
        else
            xf_chunk<Tout, VEC, true>(xf, nullptr, nullptr, vin, vout, 0u);
        *reinterpret_cast<Vout*>(out + t * VEC) = vout;
    }
}

// ---------------------------------------------------------------------------
// Tiled gather core (identity / cast / affine share it).
//
// A persistent grid of waves loops over TILES of consecutive output rows.
// Per tile, lane L of the wave loads idx[row0 + L] (one coalesced load for up
// to 64 rows), resolves the owner and forms the row's source address ONCE
// (the only 64-bit arithmetic), and the wave then sweeps the tile's chunks
// in passes of 64 lanes: chunk j = pass * 64 + lane belongs to tile row
// j / cpr, whose source address comes from that row's lane by a wave
// shuffle. (row, chunk-in-row) advance incrementally per pass, so the loop
// has no division and all per-chunk arithmetic is 32-bit. U passes are
// issued back to back before the first convert/store: U * INB bytes per lane
// in flight (f32->bf16: 4 passes = 8 dwordx4 loads, 16 rows per wave). The
// next tile's indices are fetched before the current payload is waited on.
// The store side stays exactly 16 B per lane, contiguous across the wave.
//
// Directory: for nparts <= DDS_DIR_KPARTS it arrives BY VALUE in the kernel
// arguments (scalar registers: no global loads, no LDS staging, no barrier);
// the host pads prefix[k >= nparts] with the total, so the unrolled compare
// chain `prefix[k] <= g` picks the largest k < nparts with prefix[k] <= g,
// exactly what owner_of's binary search returns (empty parts included).
// LDSDIR = true keeps the LDS-staged directory for larger worlds, paid once
// per persistent block.
//
// Measured (MI355X, flagship 262,144 x 512-B f32 rows -> bf16; 2048 blocks,
// 16-row tiles = one group of 4 passes, 2 tiles per wave, nontemporal
// stores): kernel 43.9 -> 38.5 us, 4.63 -> 5.28 TB/s r+w
// (profiles/gather_tiled_ab.txt).
// ---------------------------------------------------------------------------
typedef uint32_t dds_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t dds_u32x2 __attribute__((ext_vector_type(2)));
#define DDS_GLOBAL_AS __attribute__((address_space(1)))

// The packed output is written once and not read back by the gather, so it
// is stored NON-TEMPORAL: measured on MI355X at the flagship shape (262,144
// x 512-B f32 rows -> bf16, 4 rotating 64-MiB outputs) plain stores 42.96 us,
// nontemporal stores 38.50 us per step; nontemporal LOADS of the payload
// 40.20 us alone and 39.40 us together with the stores, so loads stay plain
// (profiles/gather_tiled_ab.txt).
template <typename V>
__device__ __forceinline__ void store_out(V* p, const V& v) {
    static_assert(sizeof(V) == 16, "store side is exactly 16 B per lane");
    dds_u32x4 w;
    __builtin_memcpy(&w, &v, 16);
    __builtin_nontemporal_store(w, reinterpret_cast<dds_u32x4*>(p));
}

// Load sizeof(V) bytes through an explicit GLOBAL pointer: the address went
// through a wave shuffle as an integer, so the compiler would otherwise emit
// flat_load (which also occupies lgkmcnt).
template <typename V>
__device__ __forceinline__ V load_global(uintptr_t a) {
    constexpr int B = sizeof(V);
    V r;
    if constexpr (B % 16 == 0) {
        dds_u32x4 w[B / 16];
#pragma unroll
        for (int i = 0; i < B / 16; ++i)
            w[i] = ((const DDS_GLOBAL_AS dds_u32x4*)a)[i];
        __builtin_memcpy(&r, w, B);
    } else if constexpr (B == 8) {
        const dds_u32x2 w = *(const DDS_GLOBAL_AS dds_u32x2*)a;
        __builtin_memcpy(&r, &w, B);
    } else if constexpr (B == 4) {
        const uint32_t w = *(const DDS_GLOBAL_AS uint32_t*)a;
        __builtin_memcpy(&r, &w, B);
    } else {
        static_assert(B == 2, "unsupported vector size");
        const uint16_t w = *(const DDS_GLOBAL_AS uint16_t*)a;
        __builtin_memcpy(&r, &w, B);
    }
    return r;
}

// passes issued back to back: ~128 B per lane in flight, 1..8 passes
template <int INB>
constexpr int tiled_unroll() {
    return INB >= 128 ? 1 : (128 / INB > 8 ? 8 : 128 / INB);
}

// What k_gather_tiled keeps for a column transform: the scales and shifts of
// the U chunks in flight. Empty for every other transform, so those
// instantiations carry nothing of it.
template <typename Xf, int VEC, int U, bool = Xf::kNeedsCol>
struct TiledCols {};
template <typename Xf, int VEC, int U>
struct TiledCols<Xf, VEC, U, true> {
    VecT<float, VEC> s[U], h[U];
};

template <typename Tin, typename Tout, typename Xf, bool LDSDIR>
__global__ void __launch_bounds__(kBlock)
k_gather_tiled(const GatherDirK dir, const void* const* peer_base,
               const int64_t* gprefix, int nparts,
               const int64_t* __restrict__ idx, int64_t nidx, int64_t ntiles,
               uint32_t cpr, uint32_t tile_rows, Xf xf,
               Tout* __restrict__ out, unsigned long long* oob) {
    constexpr int VEC = 16 / sizeof(Tout);
    constexpr int INB = VEC * sizeof(Tin);
    constexpr int U = tiled_unroll<INB>();
    using Vin = VecT<Tin, VEC>;
    using Vout = VecT<Tout, VEC>;
    __shared__ LdsDir<uintptr_t> ldir;  // unused, so not allocated, without LDSDIR
    if constexpr (LDSDIR) ldir.load(peer_base, nparts, gprefix);
    const int64_t total = LDSDIR ? ldir.prefix[0][nparts] : dir.prefix[DDS_DIR_KPARTS];
    TiledCols<Xf, VEC, U> tc;  // an empty object unless xf wants columns

    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t wstride = (int64_t)gridDim.x * (kBlock / 64);
    int64_t tile = (int64_t)blockIdx.x * (kBlock / 64) + wave;
    if (tile >= ntiles) return;

    // chunk j of a tile -> (row-in-tile, chunk-in-row); a tile starts on a
    // row boundary, so the walk starts from (lane / cpr, lane % cpr) in every
    // tile and advances by 64 chunks per pass
    const uint32_t q64 = 64u / cpr, r64 = 64u % cpr;
    const uint32_t rl0 = lane / cpr, c0 = lane - rl0 * cpr;
    const int64_t row_bytes = (int64_t)cpr * INB;

    int64_t g_next = 0;
    {
        const int64_t r = tile * tile_rows + lane;
        if (lane < tile_rows && r < nidx) g_next = idx[r];
    }
    for (; tile < ntiles; tile += wstride) {
        const int64_t row0 = tile * tile_rows;
        const int64_t left = nidx - row0;
        const uint32_t nrows = left < (int64_t)tile_rows ? (uint32_t)left : tile_rows;
        const int64_t g = g_next;
        if (tile + wstride < ntiles) {  // next tile's indices, ahead of the payload
            const int64_t r = (tile + wstride) * tile_rows + lane;
            if (lane < tile_rows && r < nidx) g_next = idx[r];
        }
        // per-row work, once: bounds, owner, source address (0 = skip)
        uintptr_t src = 0;
        if (lane < nrows) {
            if (g < 0 || g >= total) {
                atomicAdd(oob, 1ull);
            } else if constexpr (LDSDIR) {
                const int p = owner_of(ldir, nparts, g);
                src = ldir.base[p] + (uintptr_t)((g - ldir.prefix[0][p]) * row_bytes);
            } else {
                int64_t pf = dir.prefix[0];
                uintptr_t bs = reinterpret_cast<uintptr_t>(dir.base[0]);
#pragma unroll
                for (int k = 1; k < DDS_DIR_KPARTS; ++k) {
                    const bool ge = dir.prefix[k] <= g;
                    pf = ge ? dir.prefix[k] : pf;
                    bs = ge ? reinterpret_cast<uintptr_t>(dir.base[k]) : bs;
                }
                src = bs + (uintptr_t)((g - pf) * row_bytes);
            }
        }
        Vout* __restrict__ op = reinterpret_cast<Vout*>(out) + row0 * cpr;
        const uint32_t nch = nrows * cpr;
        // a tile without skipped rows runs its full groups branch-free: the
        // U passes' loads are then issued back to back and waited on with
        // counted vmcnt (loads behind per-lane branches make the compiler
        // wait for ALL outstanding loads before each next one)
        const bool clean = __ballot(lane < nrows && src == 0) == 0;
        uint32_t rl = rl0, c = c0;
        for (uint32_t jb = 0; jb < nch; jb += 64u * U) {  // wave-uniform
            if (clean && jb + 64u * U <= nch) {
                Vin vin[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const uintptr_t sp =
                        (uintptr_t)__shfl((unsigned long long)src, (int)(rl & 63u));
                    // A column transform's scales and shifts are fetched AHEAD
                    // of the payload: loads return in order, so a vector load
                    // issued at the convert would wait for every payload load.
                    if constexpr (Xf::kNeedsCol) {
                        tc.s[u] = *reinterpret_cast<const VecT<float, VEC>*>(xf.scale + c * VEC);
                        tc.h[u] = *reinterpret_cast<const VecT<float, VEC>*>(xf.shift + c * VEC);
                    }
                    vin[u] = load_global<Vin>(sp + (uintptr_t)(c * (uint32_t)INB));
                    c += r64;
                    rl += q64;
                    if (c >= cpr) {
                        c -= cpr;
                        rl += 1;
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    Vout vout;
                    if constexpr (Xf::kNeedsCol) {
#pragma unroll
                        for (int k = 0; k < VEC; ++k)
                            vout.v[k] = xf.template apply<Tout>(vin[u].v[k], tc.s[u].v[k],
                                                                tc.h[u].v[k]);
                    } else {
#pragma unroll
                        for (int k = 0; k < VEC; ++k)
                            vout.v[k] = xf.template apply<Tout>(vin[u].v[k]);
                    }
                    store_out(&op[jb + 64u * u + lane], vout);
                }
            } else {
                // partial group or a tile with skipped rows: one pass at a
                // time, load and store under the same per-lane predicate
#pragma unroll 1
                for (int u = 0; u < U; ++u) {
                    const uint32_t j = jb + 64u * u + lane;
                    // every lane takes part in the shuffle
                    const uintptr_t sp =
                        (uintptr_t)__shfl((unsigned long long)src, (int)(rl & 63u));
                    if (j < nch && sp != 0) {
                        const Vin v =
                            load_global<Vin>(sp + (uintptr_t)(c * (uint32_t)INB));
                        Vout vout;
                        if constexpr (Xf::kNeedsCol) {
                            xf_chunk<Tout, VEC, true>(xf, xf.scale, xf.shift, v, vout,
                                                      c * (uint32_t)VEC);
                        } else {
#pragma unroll
                            for (int k = 0; k < VEC; ++k)
                                vout.v[k] = xf.template apply<Tout>(v.v[k]);
                        }
                        store_out(&op[j], vout);
                    }
                    c += r64;
                    rl += q64;
                    if (c >= cpr) {
                        c -= cpr;
                        rl += 1;
                    }
                }
            }
        }
    }
}

// Per-sample lengths for a CSR gather plan: lens[i] = goff[idx[i]+1] -
// goff[idx[i]] (one kernel instead of the 3-4 elementwise torch launches
// the equivalent `goff[idx+1]-goff[idx]` costs per step).
__global__ void __launch_bounds__(kBlock)
k_csr_lens(const int64_t* goff, const int64_t* idx, int64_t nidx, int64_t nsamples,
           int64_t* __restrict__ lens, unsigned long long* oob,
           unsigned long long* elems) {
    int64_t acc = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nidx;
         i += (int64_t)gridDim.x * kBlock) {
        const int64_t g = idx[i];
        if (g < 0 || g >= nsamples) {
            lens[i] = 0;
            if (oob) atomicAdd(oob, 1ull);  // null: the gather behind counts it
            continue;
        }
        const int64_t L = goff[g + 1] - goff[g];
        lens[i] = L;
        acc += L;
    }
    if (elems) {
        // wave-reduce (64-wide) then one atomic per wave: exact gathered-
        // element stats without per-thread atomic contention
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
        if ((threadIdx.x & 63) == 0 && acc)
            atomicAdd(elems, (unsigned long long)acc);
    }
}

// Copy nd dwords src->dst by `nthreads` cooperating threads (tid strided),
// with the STORE side aligned up to dwordx4 (store width is the side the
// memory system cannot split -- same measured rule as the cast kernels):
// head dwords to 16-B store alignment, then a uint4-store body fed by four
// dword loads, then the tail dwords. Sample payload starts are only
// 4-B-granular, so the load side cannot be 16-B aligned as well. Measured
// against two other bodies (A/B r2, G samples/s): dword loads 1.845,
// align(4) dwordx4 loads (which gfx950 allows) 1.802, those plus nontemporal
// stores 1.773 -- wider loads buy nothing here, so the plain ones are used.
__device__ __forceinline__ void copy_dwords_store16(
    uint32_t* __restrict__ dst, const uint32_t* __restrict__ src,
    int64_t nd, int tid, int nthreads) {
    const int64_t h_align = (int64_t)((4 - ((((uintptr_t)dst) >> 2) & 3)) & 3);
    const int64_t h = h_align < nd ? h_align : nd;
    for (int64_t i = tid; i < h; i += nthreads) dst[i] = src[i];
    const int64_t nb = (nd - h) >> 2;
    uint4* d4 = reinterpret_cast<uint4*>(dst + h);
    const uint32_t* s2 = src + h;
    for (int64_t i = tid; i < nb; i += nthreads) {
        uint4 o;
        o.x = s2[4 * i];
        o.y = s2[4 * i + 1];
        o.z = s2[4 * i + 2];
        o.w = s2[4 * i + 3];
        d4[i] = o;
    }
    for (int64_t i = h + (nb << 2) + tid; i < nd; i += nthreads) dst[i] = src[i];
}

// Copy n units of type U by `nthreads` cooperating threads: dwords go
// through the store-aligning copy above, uint4 and bytes one unit per thread.
template <typename U>
__device__ __forceinline__ void copy_units(U* dst, const U* src, int64_t n, int tid,
                                           int nthreads) {
    if constexpr (std::is_same_v<U, uint32_t>) {
        copy_dwords_store16(dst, src, n, tid, nthreads);
    } else {
        for (int64_t c = tid; c < n; c += nthreads) dst[c] = src[c];
    }
}

// ---------------------------------------------------------------------------
// CSR gather, per sample: GROUP lanes cooperate per sample (see gather_csr's
// heuristic note; small groups amortize per-sample setup across the wave --
// 16 for small samples so many samples stay in flight per CU, 64 or the whole
// block for larger payloads). U is the copy unit: uint4 for 16-B-granular
// elements, uint32_t for 4-B-granular ones (dword addressing with
// 16-B-aligned stores), uint8_t for the rest.
// ---------------------------------------------------------------------------
template <typename U, int GROUP>
__global__ void __launch_bounds__(kBlock)
k_gather_csr_wave(const void* const* peer_base,
                  const int64_t* sample_prefix, const int64_t* elem_prefix, int nparts,
                  const int64_t* goff,
                  const int64_t* idx, int64_t nidx,
                  const int64_t* out_off, int64_t units_per_elem,
                  int64_t cap_elems,
                  U* __restrict__ out, unsigned long long* ctrs) {
    __shared__ LdsDir<const U*, 2> dir;
    dir.load(peer_base, nparts, sample_prefix, elem_prefix);

    constexpr int GPB = kBlock / GROUP;  // sample groups per block
    const int64_t first = (int64_t)blockIdx.x * GPB + threadIdx.x / GROUP;
    const int64_t step = (int64_t)gridDim.x * GPB;
    const int tid = threadIdx.x % GROUP;
    for (int64_t s = first; s < nidx; s += step) {
        const int64_t g = idx[s];
        if (out_of_range(dir, nparts, g)) {
            if (tid == 0) atomicAdd(ctrs + DDS_CTR_OOB, 1ull);
            continue;
        }
        const int p = owner_of(dir, nparts, g);
        const int64_t e0 = goff[g];
        const int64_t len = goff[g + 1] - e0;
        const int64_t o0 = out_off[s];
        if (len <= 0) continue;  // an empty sample: nothing to write or skip
        if (o0 < 0 || o0 + len > cap_elems) {  // undersized capacity buffer:
            if (tid == 0) {                    // never write OOB
                atomicAdd(ctrs + DDS_CTR_CAP, 1ull);
                // keep the true-bytes counter honest (see k_csr_plan2)
                atomicAdd(ctrs + DDS_CTR_ELEMS,
                          (unsigned long long)(-(long long)len));
            }
            continue;
        }
        copy_units<U>(out + o0 * units_per_elem,
                      dir.base[p] + (e0 - dir.prefix[1][p]) * units_per_elem,
                      len * units_per_elem, tid, GROUP);
    }
}

// ---------------------------------------------------------------------------
// CSR plan: per-sample lens + exclusive scan -> out_off, PLUS a balanced
// work-item list for the gather.
//
// History of this path (all measured at B=262144, ~512 B mean samples):
//   r1: zeros + lens kernel + torch cumsum               ~25 us plan
//   r2a: single fused lens+scan+gather kernel            2x SLOWER overall
//        (block-wide phase barriers serialize the payload copies)
//   r2b: decoupled-lookback scan kernel                  57-83 us (the
//        cross-tile flag traffic dominates regardless of spin flavor)
//   r2c (this): THREE tiny deterministic kernels, no cross-block waiting:
//        k_csr_plan1  per-tile lens + block scan -> partial out_off,
//                     per-tile (elems, items) aggregates
//        k_csr_plan2  one block scans the tile aggregates -> bases, totals
//        k_csr_plan3  finalize out_off (+tile base), capacity check, and
//                     EMIT work items: samples are split into <=ITEM-element
//                     pieces so every gather group gets near-uniform work
//                     (static sample-per-group scheduling loses ~1.5x to
//                     the max-of-4-samples-per-wave effect; fixed-len A/B
//                     r2: 46 vs 75 us for the same mean bytes).
//
// Item descriptor: (sample_index << 20) | piece_index (piece < 2^20 =>
// samples up to 2^20 * ITEM elements; guarded in plan3).
// Scratch layout (csr_plan_scratch_bytes): [aggs 2*ntiles][lens nidx]
// [meta 2] int64 each; meta = {total_items, total_elems}.
// ---------------------------------------------------------------------------
// Work-item size: A/B on MI355X (B=262144, 16..240-elem f32 samples), with
// self-contained descriptors: 256 B -> 2.39G, 512 B -> 2.65G, 1024 B ->
// 2.91G samples/s -- per-item fixed cost beats the wave-balance gain, so
// items hold most whole samples and splitting only trims outliers.
// Also tried and REVERTED (commit history has both sides): (a) fusing the
// aggregate scan into plan1's last block -- the per-block __threadfence
// costs an L2 writeback each, plan1 8 -> 41 us; (b) size-banded item
// emission for wave uniformity -- the per-block same-address atomicAdd
// allocation serializes at ~60 ns/op (plan3 6 -> 58 us) AND the banded
// dst scatter loses write locality (gather 76 -> 85 us).
constexpr int kItemBytes = 1024;  // env override: DDSTORE_CSR_ITEM

__device__ __forceinline__ void block_scan_pair(int64_t& x, int64_t& y,
                                                int64_t* s_wsum2, int lane,
                                                int wave, int64_t* tile_tot) {
    // inclusive block scan of (x, y) over kBlock threads (wave shfl + LDS)
    for (int off = 1; off < 64; off <<= 1) {
        int64_t ax = __shfl_up(x, off);
        int64_t ay = __shfl_up(y, off);
        if (lane >= off) {
            x += ax;
            y += ay;
        }
    }
    if (lane == 63) {
        s_wsum2[2 * wave] = x;
        s_wsum2[2 * wave + 1] = y;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t ax = 0, ay = 0;
        for (int w = 0; w < kBlock / 64; ++w) {
            int64_t tx = s_wsum2[2 * w], ty = s_wsum2[2 * w + 1];
            s_wsum2[2 * w] = ax;
            s_wsum2[2 * w + 1] = ay;
            ax += tx;
            ay += ty;
        }
        if (tile_tot) {
            tile_tot[0] = ax;
            tile_tot[1] = ay;
        }
    }
    __syncthreads();
    x += s_wsum2[2 * wave];
    y += s_wsum2[2 * wave + 1];
}

__global__ void __launch_bounds__(kBlock)
k_csr_plan1(const int64_t* goff, int64_t nsamples,
            const int64_t* idx, int64_t nidx, int64_t item_elems,
            int64_t* __restrict__ lens_tmp, int64_t* __restrict__ e0_tmp,
            int64_t* __restrict__ aggs, unsigned long long* ctrs) {
    __shared__ int64_t s_wsum2[2 * (kBlock / 64)];
    __shared__ int64_t s_tot[2];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t ntiles = (nidx + kBlock - 1) / kBlock;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t i = tile * kBlock + threadIdx.x;
        int64_t L = 0, e0 = -1;
        if (i < nidx) {
            const int64_t g = idx[i];
            if (g < 0 || g >= nsamples) {
                atomicAdd(ctrs + DDS_CTR_OOB, 1ull);
            } else {
                e0 = goff[g];
                L = goff[g + 1] - e0;
            }
            lens_tmp[i] = L;
            e0_tmp[i] = e0;  // global element start (src side), cached for plan3
        }
        int64_t x = L;
        int64_t y = L > 0 ? (L + item_elems - 1) / item_elems : 0;
        block_scan_pair(x, y, s_wsum2, lane, wave, s_tot);
        // (out_off is written complete, with bases, by plan3)
        if (threadIdx.x == 0) {
            aggs[2 * tile] = s_tot[0];
            aggs[2 * tile + 1] = s_tot[1];
        }
        __syncthreads();  // LDS reused next tile
    }
}

__global__ void __launch_bounds__(kBlock)
k_csr_plan2(int64_t* __restrict__ aggs, int64_t ntiles,
            int64_t* __restrict__ meta, unsigned long long* ctrs) {
    // ONE block: running exclusive scan of the (elems, items) tile
    // aggregates in chunks of kBlock; writes totals into meta
    __shared__ int64_t s_wsum2[2 * (kBlock / 64)];
    __shared__ int64_t s_tot[2];
    __shared__ int64_t s_carry[2];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) {
        s_carry[0] = 0;
        s_carry[1] = 0;
    }
    __syncthreads();
    for (int64_t base = 0; base < ntiles; base += kBlock) {
        const int64_t t = base + threadIdx.x;
        int64_t x = t < ntiles ? aggs[2 * t] : 0;
        int64_t y = t < ntiles ? aggs[2 * t + 1] : 0;
        const int64_t mx = x, my = y;
        block_scan_pair(x, y, s_wsum2, lane, wave, s_tot);
        if (t < ntiles) {
            aggs[2 * t] = s_carry[0] + x - mx;      // exclusive base
            aggs[2 * t + 1] = s_carry[1] + y - my;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            s_carry[0] += s_tot[0];
            s_carry[1] += s_tot[1];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        meta[0] = s_carry[1];  // total items
        meta[1] = s_carry[0];  // total elems
        // true-bytes stats: requested elements (plan3 subtracts lens of
        // capacity-skipped samples)
        atomicAdd(ctrs + DDS_CTR_ELEMS, (unsigned long long)s_carry[0]);
    }
}

// plan3 emits SELF-CONTAINED item descriptors (2 int64 each) so the gather
// does zero random metadata loads (per-item idx/goff/out_off/owner lookups
// were measured to cost MORE than the imbalance they fixed: 110 vs 75 us):
//   desc[2j]   = (peer << 56) | src_unit_offset   (units: dwords or bytes)
//   desc[2j+1] = (n_units << 44) | dst_unit_offset
// Contract with k_gather_csr_items: desc is uninitialised memory, and the
// item total in meta[0] (scanned before the capacity check) counts the slots
// of skipped samples too. So every slot j < min(meta[0], desc_cap) is written
// here in the same call -- a kept sample's pieces, or (0, 0) = zero units for
// a skipped one -- and the gather reads no slot at or beyond that bound. A
// kept sample's slots always lie below desc_cap (sum of ceil(L / item_elems)
// over samples that fit cap_elems <= cap_elems / item_elems + nidx).
static_assert(DDS_MAX_PARTS <= 128,
              "the owner travels as p << 56 in a signed 64-bit descriptor and comes "
              "back as (int)(d0 >> 56): 127 is the largest owner that keeps it "
              "non-negative");
__global__ void __launch_bounds__(kBlock)
k_csr_plan3(const int64_t* __restrict__ lens_tmp,
            const int64_t* __restrict__ e0_tmp, int64_t nidx,
            const int64_t* sample_prefix, const int64_t* elem_prefix,
            int nparts, const int64_t* idx,
            int64_t item_elems, int64_t units_per_elem, int64_t cap_elems,
            const int64_t* __restrict__ aggs,
            int64_t* __restrict__ out_off,
            int64_t* __restrict__ desc, int64_t desc_cap,
            unsigned long long* ctrs) {
    __shared__ int64_t s_wsum2[2 * (kBlock / 64)];
    __shared__ int64_t s_sprefix[DDS_MAX_PARTS + 1];
    __shared__ int64_t s_eprefix[DDS_MAX_PARTS + 1];
    for (int i = threadIdx.x; i <= nparts; i += kBlock) {
        s_sprefix[i] = sample_prefix[i];
        s_eprefix[i] = elem_prefix[i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t ntiles = (nidx + kBlock - 1) / kBlock;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t i = tile * kBlock + threadIdx.x;
        const int64_t L = i < nidx ? lens_tmp[i] : 0;
        int64_t x = L;
        int64_t items = L > 0 ? (L + item_elems - 1) / item_elems : 0;
        int64_t y = items;
        block_scan_pair(x, y, s_wsum2, lane, wave, nullptr);
        const int64_t e_base = aggs[2 * tile], i_base = aggs[2 * tile + 1];
        if (i < nidx) {
            const int64_t excl_e = e_base + x - L;   // global elem offset
            const int64_t excl_i = i_base + y - items;
            out_off[i + 1] = e_base + x;
            if (i == 0) out_off[0] = 0;
            if (L > 0) {
                if (excl_e + L > cap_elems ||
                    excl_i + items > desc_cap ||
                    L * units_per_elem >= (int64_t(1) << 44)) {
                    // over-capacity (or pathological): nothing of the
                    // sample is written; counted. Its slots are still part
                    // of the scanned item total, so those below desc_cap
                    // get zero-length descriptors (see the contract above)
                    atomicAdd(ctrs + DDS_CTR_CAP, 1ull);
                    atomicAdd(ctrs + DDS_CTR_ELEMS,
                              (unsigned long long)(-(long long)L));
                    const int64_t end =
                        items < desc_cap - excl_i ? excl_i + items : desc_cap;
                    for (int64_t j = excl_i; j < end; ++j) {
                        desc[2 * j] = 0;
                        desc[2 * j + 1] = 0;
                    }
                } else {
                    const int64_t g = idx[i];
                    const int64_t p = owner_of(s_sprefix, nparts, g);
                    const int64_t src0 =
                        (e0_tmp[i] - s_eprefix[p]) * units_per_elem;
                    const int64_t dst0 = excl_e * units_per_elem;
                    const int64_t iu = item_elems * units_per_elem;
                    const int64_t nu = L * units_per_elem;
                    for (int64_t k = 0; k < items; ++k) {
                        const int64_t off = k * iu;
                        const int64_t n = nu - off < iu ? nu - off : iu;
                        desc[2 * (excl_i + k)] = (p << 56) | (src0 + off);
                        desc[2 * (excl_i + k) + 1] = (n << 44) | (dst0 + off);
                    }
                }
            }
        }
        __syncthreads();
    }
}

// Balanced CSR gather: GROUP lanes per work item (one <=ITEM-byte piece of
// one sample, self-contained descriptor); near-uniform work per wave kills
// the max-of-N-samples imbalance of the per-sample kernel, and the
// coalesced 16-B descriptor read is the ONLY metadata access. Item count
// is read from meta on device (the host never syncs for it) and bounded by
// desc_cap: with skipped samples it can exceed the slots that exist, and
// only slots below min(meta[0], desc_cap) were written by k_csr_plan3.
// U is the descriptors' unit and the copy unit: uint32_t or uint8_t.
template <typename U, int GROUP>
__global__ void __launch_bounds__(kBlock)
k_gather_csr_items(const void* const* peer_base, int nparts,
                   const int64_t* __restrict__ desc,
                   const int64_t* __restrict__ meta, int64_t desc_cap,
                   U* __restrict__ out) {
    __shared__ const U* s_base[DDS_MAX_PARTS];
    for (int i = threadIdx.x; i < nparts; i += kBlock)
        s_base[i] = reinterpret_cast<const U*>(peer_base[i]);
    __syncthreads();
    const int64_t total = meta[0] < desc_cap ? meta[0] : desc_cap;
    constexpr int GPB = kBlock / GROUP;
    const int64_t first = (int64_t)blockIdx.x * GPB + threadIdx.x / GROUP;
    const int64_t step = (int64_t)gridDim.x * GPB;
    const int tid = threadIdx.x % GROUP;
    for (int64_t j = first; j < total; j += step) {
        const int64_t d0 = desc[2 * j];
        const int64_t d1 = desc[2 * j + 1];
        const int p = (int)(d0 >> 56);
        const int64_t src_u = d0 & ((int64_t(1) << 56) - 1);
        const int64_t n_u = d1 >> 44;
        const int64_t dst_u = d1 & ((int64_t(1) << 44) - 1);
        copy_units<U>(out + dst_u, s_base[p] + src_u, n_u, tid, GROUP);
    }
}

// Stats of one padded CSR gather: gathered elements, sum(min(len, max_len)),
// into DDS_CTR_ELEMS and bad indices into DDS_CTR_OOB. Only the first
// kPadCountBlocks blocks of the launch run this, each over a strided share of
// ALL the indices, so a launch issues at most kPadCountBlocks atomics per
// counter however large its grid is. One atomic per block of the gather grid
// is not few enough: same-address atomics serialize (plan3 note above), and
// at the CSR bench shape (B=262144: 32768 blocks, ~43 ns per atomic) they
// alone held the kernel at 1.40-1.45 ms, whatever the payload mapping and
// store flavour; with this pre-pass the same kernel takes 149 us (MI355X).
// The cost is a second read of idx and the two offsets by 64 blocks.
constexpr int kPadCountBlocks = 64;

template <typename P>
__device__ __forceinline__ void count_padded(const LdsDir<P, 2>& dir, int nparts,
                                             const int64_t* goff, const int64_t* idx,
                                             int64_t nidx, int64_t max_len,
                                             unsigned long long* s_acc,
                                             unsigned long long* ctrs) {
    const int64_t nb = gridDim.x < (unsigned)kPadCountBlocks ? gridDim.x : kPadCountBlocks;
    unsigned long long acc_elems = 0, acc_oob = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nidx;
         i += nb * kBlock) {
        const int64_t g = idx[i];
        if (out_of_range(dir, nparts, g)) {
            acc_oob += 1;
        } else {
            const int64_t len = goff[g + 1] - goff[g];
            acc_elems += (unsigned long long)(len < max_len ? len : max_len);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        acc_elems += __shfl_down(acc_elems, off);
        acc_oob += __shfl_down(acc_oob, off);
    }
    if ((threadIdx.x & 63) == 0) {
        s_acc[2 * (threadIdx.x >> 6)] = acc_elems;
        s_acc[2 * (threadIdx.x >> 6) + 1] = acc_oob;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long e = 0, o = 0;
        for (int w = 0; w < kBlock / 64; ++w) {
            e += s_acc[2 * w];
            o += s_acc[2 * w + 1];
        }
        if (e) atomicAdd(ctrs + DDS_CTR_ELEMS, e);
        if (o) atomicAdd(ctrs + DDS_CTR_OOB, o);
    }
}

// ---------------------------------------------------------------------------
// Padded CSR gather: sample idx[s] lands in row s of a dense (n, max_len,
// disp) output, cut to its first max_len elements and filled up with the pad;
// lengths[s] gets its true (uncut) length. The output offsets are s * max_len
// by construction, so there is no scan, no plan and no scratch: one launch.
//
// Mapping: lane-groups per sample, as in k_gather_csr_wave -- 2^lg_group
// lanes own one output row, resolve the sample ONCE (index, the two offsets,
// owner, source address) and sweep the row's VEC-element chunks with adds
// only. Chosen by construction over one chunk per thread on the flat output
// (k_gather_oneshot's mapping), where every thread pays the i64 divide, three
// dependent metadata loads and the LDS search for ONE chunk; the two were NOT
// ranked by an A/B -- a first chunk-per-thread version was measured only
// with per-block counter atomics, which hid everything else (see
// count_padded). Rows are all the same size on the store side, the side that
// costs, so the per-sample kernel's max-of-N imbalance does not come back:
// only the loads differ per row. The group is sized from the chunks per row
// by the host (8..64 lanes, the whole block for few long rows).
//
// Measured on MI355X at the CSR bench shape (B=262144, L=240, disp=1 f32,
// lengths 16..239: 133.7 MB payload, 251.7 MB f32 output): 149 us f32->f32
// (2.59 TB/s r+w), 120 us f32->bf16, against 96 us for the ragged get_csr
// fast path and 13.3 ms for get_csr + torch scatter (+ cast) into the same
// layout (profiles/csr_padded_ab.txt). Nontemporal 16-B stores (store_out)
// made no difference here -- 148.8/149.1 us against 148.0/149.2 plain,
// 120.4/120.9 against 121.0/120.8 for bf16 -- so the stores are plain.
//
// VEC = 16 / sizeof(Tout) keeps the store side at 16 B (store-width note at
// k_gather_oneshot). `aligned` (disp % VEC == 0): no chunk straddles the
// valid/pad boundary and source chunks are aligned (shard bases come from
// hipMalloc), so a valid chunk is one vector load. Otherwise, if the ROW
// still is a whole number of chunks, a chunk is fed by VEC element loads,
// predicated at the boundary -- 16-B stores from narrower loads, the
// arrangement copy_dwords_store16 measured best for 4-B-granular payloads;
// this is what the CSR bench shape (disp = 1) runs. VEC = 1 is the
// element-wise fallback, and the same-dtype byte move of 16-B-granular
// elements runs as XfIdentity with VEC = 1 over uint4 units. Pad chunks
// issue no load. `pad16` holds the pad's raw bits replicated over 16 B; it
// goes through neither cast nor affine.
//
// Stats: the first kPadCountBlocks blocks count before they gather (see
// count_padded); the gather loop itself touches no counter.
// ---------------------------------------------------------------------------
template <typename Tin, typename Tout, int VEC, typename Xf>
__global__ void __launch_bounds__(kBlock)
k_gather_csr_padded(const void* const* peer_base, const int64_t* sample_prefix,
                    const int64_t* elem_prefix, int nparts, const int64_t* goff,
                    const int64_t* idx, int64_t nidx, int64_t disp, int64_t max_len,
                    int lg_group, bool aligned, Xf xf, dds_u32x4 pad16,
                    Tout* __restrict__ out, int64_t* __restrict__ lengths,
                    unsigned long long* ctrs) {
    using Vin = VecT<Tin, VEC>;
    using Vout = VecT<Tout, VEC>;
    static_assert(sizeof(Vout) <= 16, "pad16 covers one output chunk");
    __shared__ LdsDir<const Tin*, 2> dir;
    __shared__ unsigned long long s_acc[2 * (kBlock / 64)];
    dir.load(peer_base, nparts, sample_prefix, elem_prefix);

    Vout vpad;
    __builtin_memcpy(&vpad, &pad16, sizeof(Vout));
    const int group = 1 << lg_group;
    const int tid = threadIdx.x & (group - 1);
    const int64_t first =
        (int64_t)blockIdx.x * (kBlock >> lg_group) + (threadIdx.x >> lg_group);
    const int64_t step = (int64_t)gridDim.x * (kBlock >> lg_group);
    const int64_t row_elems = max_len * disp;
    const int64_t cpr = row_elems / VEC;  // chunks per output row
    // Column transform: element e of a row sits in column e % disp. A lane
    // starts at chunk `tid` and steps by `group` chunks, so two divides per
    // thread set up a walk that needs only an add and a compare per chunk.
    const float* csc = nullptr;
    const float* csh = nullptr;
    uint32_t d32 = 0, col0 = 0, cstep = 0;
    if constexpr (Xf::kNeedsCol) {
        csc = xf.scale;
        csh = xf.shift;
        d32 = (uint32_t)disp;
        col0 = (uint32_t)(((uint32_t)tid * (uint32_t)VEC) % d32);
        cstep = (uint32_t)(((uint32_t)group * (uint32_t)VEC) % d32);
    }
    if (blockIdx.x < kPadCountBlocks)  // block-uniform
        count_padded(dir, nparts, goff, idx, nidx, max_len, s_acc, ctrs);
    for (int64_t s = first; s < nidx; s += step) {
        const int64_t g = idx[s];
        const Tin* sp = nullptr;
        int64_t nvalid = 0;  // valid elements at the head of the row
        if (out_of_range(dir, nparts, g)) {  // all-pad row, never read OOB
            if (tid == 0) lengths[s] = 0;
        } else {
            const int p = owner_of(dir, nparts, g);
            const int64_t e0 = goff[g];
            const int64_t len = goff[g + 1] - e0;
            const int64_t take = len < max_len ? len : max_len;
            sp = dir.base[p] + (e0 - dir.prefix[1][p]) * disp;
            nvalid = take * disp;
            if (tid == 0) lengths[s] = len;
        }
        Vout* __restrict__ op = reinterpret_cast<Vout*>(out + s * row_elems);
        uint32_t col = col0;  // column of element c * VEC, kept without a divide
        for (int64_t c = tid; c < cpr; c += group) {
            const int64_t e = c * VEC;
            Vout vout = vpad;
            if (e < nvalid) {
                if (VEC == 1 || aligned) {
                    const Vin vin = *reinterpret_cast<const Vin*>(sp + e);
                    xf_chunk<Tout, VEC, true>(xf, csc, csh, vin, vout, col);
                } else if (e + VEC <= nvalid) {
                    Vin x;
#pragma unroll
                    for (int k = 0; k < VEC; ++k) x.v[k] = sp[e + k];
                    xf_chunk<Tout, VEC, false>(xf, csc, csh, x, vout, col, d32);
                } else {  // the chunk on the valid/pad boundary
                    uint32_t cc = col;
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        if (e + k < nvalid) {
                            if constexpr (Xf::kNeedsCol)
                                vout.v[k] = xf.template apply<Tout>(sp[e + k], csc[cc],
                                                                    csh[cc]);
                            else
                                vout.v[k] = xf.template apply<Tout>(sp[e + k]);
                        }
                        if constexpr (Xf::kNeedsCol) cc = cc + 1 == d32 ? 0 : cc + 1;
                    }
                }
            }
            op[c] = vout;
            if constexpr (Xf::kNeedsCol) {
                col += cstep;
                if (col >= d32) col -= d32;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Graph-batch fetch: the edge index of a batch of graphs, relabelled to the
// packed batch, plus the batch vector. Three kernels beside the CSR gathers
// (which fetch the node features unchanged):
//   k_csr_scan3             edge offsets: plan1 + plan2 + this, no descriptors
//   k_gather_csr_relabel    the kept graphs' edges, node ids shifted by ptr[s]
//   k_graph_fill            batch segments, batch tail, edge_index tail
// Both offset arrays are monotone, so the graphs whose nodes fit
// (ptr[s+1] <= ncap) are a prefix of the request, and so are those whose
// edges are written as well (edge_ptr[s+1] <= ecap on top of that). The
// relabel kernel writes exactly the edge slots [0, edge_ptr[Ke]) of that
// second prefix and the fill kernel everything else, so every element of
// `batch` and `edge_index` is written exactly once and nothing is pre-filled.
// Measured on MI355X at the CSR bench shape with 4 edges per node (B=262144
// graphs, 33.4 M nodes of one f32, 133.7 M edges, exact capacities): the whole
// fetch 1138 us for int64 ids, 954 us int32 -> int64, 763 us int32 -> int32,
// against 4465 us for two get_csr(out=) calls + repeat_interleave + add +
// .t().contiguous() on int64 storage (profiles/graph_batch_ab.txt). The
// group size (one wave per graph) and the grids were chosen by construction
// and not swept.
// ---------------------------------------------------------------------------

// out_off[0..nidx] from plan1's per-sample lens and plan2's exclusive tile
// bases: the scan half of k_csr_plan3, with no descriptors and no capacity
// logic.
__global__ void __launch_bounds__(kBlock)
k_csr_scan3(const int64_t* __restrict__ lens_tmp, int64_t nidx,
            const int64_t* __restrict__ aggs, int64_t* __restrict__ out_off) {
    __shared__ int64_t s_wsum2[2 * (kBlock / 64)];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t ntiles = (nidx + kBlock - 1) / kBlock;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t i = tile * kBlock + threadIdx.x;
        int64_t x = i < nidx ? lens_tmp[i] : 0;
        int64_t y = 0;
        block_scan_pair(x, y, s_wsum2, lane, wave, nullptr);
        if (i < nidx) {
            out_off[i + 1] = aggs[2 * tile] + x;
            if (i == 0) out_off[0] = 0;
        }
        __syncthreads();  // LDS reused next tile
    }
}

// One (src, dst) pair of node ids. Source pairs are pair-aligned (shard bases
// come from hipMalloc, rows are whole pairs); the (Ecap, 2) output is only
// promised element alignment, which is all this type claims.
template <typename T>
struct IdPair {
    T src, dst;
};

constexpr int kGraphGroup = 64;  // lanes per graph: one wave

// Relabelling edge gather: GROUP lanes per graph, resolved once per graph as
// in k_gather_csr_wave (index, bad-index test, owner, the offsets), then one
// load of a whole pair per lane (16 B for int64 ids, 8 B for int32), ptr[s]
// added to both ids, and either one pair store into (Ecap, 2) or one store
// into each row of (2, Ecap). Consecutive lanes take consecutive edges: the
// load stream and both store streams are contiguous across the group.
// A graph's edges are written iff its nodes were kept (ptr[s+1] <= ncap) and
// its edge slice ends at or before ecap. A graph with edges that are dropped
// counts once in DDS_CTR_CAP and takes its edges back out of DDS_CTR_ELEMS
// (k_csr_plan2 added the requested total), from lane 0 only -- the
// undersized-buffer path, as in k_gather_csr_wave. Bad indices were counted by
// k_csr_plan1 and have length 0 here. The tail of edge_index is written by
// k_graph_fill, not here.
template <typename Tin, typename Tout, int GROUP, bool COO>
__global__ void __launch_bounds__(kBlock)
k_gather_csr_relabel(const void* const* peer_base, const int64_t* sample_prefix,
                     const int64_t* elem_prefix, int nparts, const int64_t* goff,
                     const int64_t* idx, int64_t nidx,
                     const int64_t* __restrict__ ptr,
                     const int64_t* __restrict__ edge_ptr, int64_t ncap,
                     int64_t ecap, Tout* __restrict__ out,
                     unsigned long long* ctrs) {
    using Pin = VecT<Tin, 2>;
    __shared__ LdsDir<const Pin*, 2> dir;
    dir.load(peer_base, nparts, sample_prefix, elem_prefix);

    constexpr int GPB = kBlock / GROUP;
    const int64_t first = (int64_t)blockIdx.x * GPB + threadIdx.x / GROUP;
    const int64_t step = (int64_t)gridDim.x * GPB;
    const int tid = threadIdx.x % GROUP;
    for (int64_t s = first; s < nidx; s += step) {
        const int64_t g = idx[s];
        if (out_of_range(dir, nparts, g)) continue;  // counted by k_csr_plan1
        const int64_t o0 = edge_ptr[s];
        const int64_t len = edge_ptr[s + 1] - o0;
        if (len <= 0) continue;
        if (ptr[s + 1] > ncap || o0 < 0 || o0 + len > ecap) {
            if (tid == 0) {
                atomicAdd(ctrs + DDS_CTR_CAP, 1ull);
                atomicAdd(ctrs + DDS_CTR_ELEMS, (unsigned long long)(-(long long)len));
            }
            continue;
        }
        const Tout shift = static_cast<Tout>(ptr[s]);
        const int p = owner_of(dir, nparts, g);
        const Pin* __restrict__ sp = dir.base[p] + (goff[g] - dir.prefix[1][p]);
        for (int64_t e = tid; e < len; e += GROUP) {
            const Pin v = sp[e];
            const Tout a = static_cast<Tout>(v.v[0]) + shift;
            const Tout b = static_cast<Tout>(v.v[1]) + shift;
            if constexpr (COO) {
                out[o0 + e] = a;
                out[ecap + o0 + e] = b;
            } else {
                reinterpret_cast<IdPair<Tout>*>(out)[o0 + e] = IdPair<Tout>{a, b};
            }
        }
    }
}

// dst[0..n) = val by `nthreads` cooperating threads, the body in 16-B stores:
// head elements up to 16-B alignment, VecT body, tail (the store-width rule of
// copy_dwords_store16). dst is aligned to its element.
template <typename T>
__device__ __forceinline__ void fill_store16(T* __restrict__ dst, int64_t n, T val,
                                             int64_t tid, int64_t nthreads) {
    constexpr int V = 16 / sizeof(T);
    using Vt = VecT<T, V>;
    const int64_t h_align =
        (int64_t)(((16 - ((uintptr_t)dst & 15)) & 15) / sizeof(T));
    const int64_t h = h_align < n ? h_align : n;
    for (int64_t i = tid; i < h; i += nthreads) dst[i] = val;
    const int64_t nb = (n - h) / V;
    Vt vv;
#pragma unroll
    for (int k = 0; k < V; ++k) vv.v[k] = val;
    Vt* d = reinterpret_cast<Vt*>(dst + h);
    for (int64_t i = tid; i < nb; i += nthreads) d[i] = vv;
    for (int64_t i = h + nb * V + tid; i < n; i += nthreads) dst[i] = val;
}

// Largest k in [0, n] with a[k] <= cap, for a monotone a[0..n] with a[0] = 0
// and cap >= 0, found by the whole block: every round samples the candidate
// range at kBlock points and keeps the one stride that holds the answer
// (three rounds for 2^24 entries, one load per thread and round). Returns
// the same k in every thread.
__device__ __forceinline__ int64_t block_last_le(const int64_t* __restrict__ a,
                                                 int64_t n, int64_t cap) {
    int64_t lo = 0, hi = n;
    while (hi > lo) {  // block-uniform
        const int64_t m = hi - lo + 1;
        const int64_t stride = (m + kBlock - 1) / kBlock;
        const int64_t q = lo + (int64_t)threadIdx.x * stride;
        const int c = __syncthreads_count(q <= hi && a[q] <= cap);  // >= 1
        const int64_t nlo = lo + (int64_t)(c - 1) * stride;
        const int64_t nhi = nlo + stride - 1;
        lo = nlo;
        hi = nhi < hi ? nhi : hi;
    }
    return lo;
}

// Everything of a graph batch that is not a kept edge, in one launch and
// without atomics (a separate kernel, not folded into the relabel gather):
//   batch[ptr[s] .. ptr[s+1]) = s       for the Kn graphs whose nodes fit,
//                                       GROUP lanes per graph
//   batch[ptr[Kn] .. ncap)    = nidx    the dummy segment
//   edge_index slots of edges [edge_ptr[Ke], ecap) = fill, in both rows of
//   (2, Ecap) or as one run of (Ecap, 2)
// Kn and Ke are the kept prefixes (see the section note), found once per
// block by block_last_le over ptr and edge_ptr; no per-element search.
template <typename Tout, int GROUP>
__global__ void __launch_bounds__(kBlock)
k_graph_fill(const int64_t* __restrict__ ptr, const int64_t* __restrict__ edge_ptr,
             int64_t nidx, int64_t ncap, int64_t ecap, bool coo, Tout fill,
             int64_t* __restrict__ batch, Tout* __restrict__ edge_out) {
    const int64_t kn = block_last_le(ptr, nidx, ncap);
    const int64_t ke_all = block_last_le(edge_ptr, nidx, ecap);
    const int64_t ke = ke_all < kn ? ke_all : kn;
    const int64_t node_end = ptr[kn];
    const int64_t edge_end = edge_ptr[ke];

    constexpr int GPB = kBlock / GROUP;
    const int tid = threadIdx.x % GROUP;
    for (int64_t s = (int64_t)blockIdx.x * GPB + threadIdx.x / GROUP; s < kn;
         s += (int64_t)gridDim.x * GPB) {
        const int64_t o0 = ptr[s];
        fill_store16<int64_t>(batch + o0, ptr[s + 1] - o0, s, tid, GROUP);
    }
    const int64_t gt = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t nt = (int64_t)gridDim.x * kBlock;
    fill_store16<int64_t>(batch + node_end, ncap - node_end, nidx, gt, nt);
    if (coo) {
        fill_store16<Tout>(edge_out + edge_end, ecap - edge_end, fill, gt, nt);
        fill_store16<Tout>(edge_out + ecap + edge_end, ecap - edge_end, fill, gt, nt);
    } else {
        fill_store16<Tout>(edge_out + 2 * edge_end, 2 * (ecap - edge_end), fill, gt, nt);
    }
}

// ---------------------------------------------------------------------------
// Local scatter (reshuffle placement): row r of src -> local row
// local_idx[r] of base. Same chunk mapping as gather.
// ---------------------------------------------------------------------------
// V is the chunk a thread moves: 32 B, 16 B, or single bytes.
template <typename V>
__global__ void __launch_bounds__(kBlock)
k_scatter_rows(V* __restrict__ base, int64_t nrows, int64_t chunks_per_row,
               const int64_t* local_idx, int64_t nidx,
               const V* __restrict__ src, unsigned long long* oob) {
    const int64_t total = nidx * chunks_per_row;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * kBlock) {
        const int64_t r = t / chunks_per_row;
        const int64_t c = t - r * chunks_per_row;
        const int64_t l = local_idx[r];
        if (l < 0 || l >= nrows) {
            if (c == 0) atomicAdd(oob, 1ull);
            continue;
        }
        base[l * chunks_per_row + c] = src[t];
    }
}

// ---------------------------------------------------------------------------
// Column statistics of the local shard: per column of the row-major (R, D)
// view, the mean, the centred sum of squares M2, min and max, all in f64.
//
// Numerics: shifted sums. Every column has a pivot p -- the median of its
// values in rows 0, R/2 and R-1 (0 if that is not finite) -- and the kernel
// accumulates S1 = sum(x - p) and S2 = sum((x - p)^2). Then mean = p + S1/n
// and M2 = S2 - S1^2/n, whose cancellation is 1 + (mean - p)^2/var: a small
// number for a pivot taken from the data, however large the mean is against
// the spread (the raw-moment form has (mean/std)^2 there). A constant column
// has x - p == 0 everywhere, so M2 == 0 exactly. All blocks use the same
// pivots, so partials combine by plain addition, in a fixed order: two calls
// give the same bits. No floating-point atomics anywhere.
//
// NaN: v_min_f64/v_max_f64 drop NaNs, so every slot keeps a NaN flag; after
// the loop a flagged slot's min and max become NaN, and every later combine
// step propagates a NaN. The sums turn NaN by themselves. (Deciding from the
// sum alone would also call a column with +inf and -inf a NaN column.)
//
// Mapping: the shard is one flat array of N = R * D elements, read in chunks
// of VEC elements (16 B; 8 B for 1-byte types, which caps a thread at 8
// slots). Active thread t of S takes chunks t, t + S, t + 2S, ...; S is a
// multiple of D / gcd(D, VEC), so S * VEC is a multiple of D and slot j of
// thread t only ever sees column (t * VEC + j) % D: five f64 registers per
// slot (pivot, S1, S2, min, max), no column arithmetic in the loop. Chunks
// are aligned in the flat view whatever D is (D = 3 of f32 loads dwordx4).
// The grid has at least D / gcd(D, VEC) threads; for a D beyond the
// 256 * VEC positions one block covers, blocks own different column ranges
// (a whole image per row: 150528 u8 columns over 74 blocks).
//
// Per block: the 256 * VEC slots are folded in LDS by column with a fixed
// tree (slots e, e + D, e + 2D, ... share a column), leaving nb = min(D,
// 256 * VEC) entries; entry e of block b is column (b * 256 * VEC + e) % D.
// k_colstats_final folds the blocks of each column in block order and
// finalizes. Scratch: colstats_scratch_bytes = blocks * nb * 4 doubles,
// independent of R.
//
// Measured on MI355X, 4 GiB f32 shard of 128 columns: 1.0 ms per call with
// the read-back, 4.3 TB/s read, fixed-stride and CSR alike; torch.var_mean +
// torch.aminmax over a .double() copy: 9.2 ms and 8.1 GiB extra
// (profiles/colnorm_ab.txt). The grid (4 blocks per CU, U = 4 loads in
// flight) was chosen by construction and not swept.
// ---------------------------------------------------------------------------
template <typename T>
constexpr int stat_vec() {
    return sizeof(T) == 1 ? 8 : 16 / (int)sizeof(T);
}

template <typename T>
__device__ __forceinline__ double stat_f64(T v) {
    if constexpr (std::is_same_v<T, __half>) return (double)__half2float(v);
    else if constexpr (std::is_same_v<T, __hip_bfloat16>) return (double)__bfloat162float(v);
    else if constexpr (is_fp8_v<T>) return (double)static_cast<float>(v);
    else return (double)v;  // i64 rounds to nearest
}

template <typename T>
__device__ __forceinline__ double stat_pivot(const T* __restrict__ base, int64_t R,
                                             int64_t D, int64_t c) {
    const double a = stat_f64(base[c]);
    const double b = stat_f64(base[(R / 2) * D + c]);
    const double d = stat_f64(base[(R - 1) * D + c]);
    const double m = fmax(fmin(a, b), fmin(fmax(a, b), d));
    return fabs(m) <= 1.7976931348623157e308 ? m : 0.0;  // a NaN fails too
}

// quantity Q of a partial: 0 = S1, 1 = S2 (sums), 2 = min, 3 = max (a NaN in
// either operand stays)
template <int Q>
__device__ __forceinline__ double stat_combine(double a, double b) {
    if constexpr (Q < 2) {
        return a + b;
    } else {
        const double r = Q == 2 ? fmin(a, b) : fmax(a, b);
        return (a != a || b != b) ? __builtin_nan("") : r;
    }
}

template <int Q>
__device__ __forceinline__ double stat_identity() {
    return Q < 2 ? 0.0 : (Q == 2 ? __builtin_inf() : -__builtin_inf());
}

// Fold quantity Q of the block's 256 * VEC slots by column and write the nb
// entries of this block.
template <int Q, int VEC>
__device__ __forceinline__ void stat_block_fold(double* s_stage, const double (&val)[VEC],
                                                int64_t D, int64_t nb,
                                                double* __restrict__ part) {
    constexpr int64_t W = (int64_t)kBlock * VEC;
    __syncthreads();  // the previous quantity has been read
#pragma unroll
    for (int j = 0; j < VEC; ++j) s_stage[threadIdx.x * VEC + j] = val[j];
    __syncthreads();
    if (D < W) {  // block-uniform
        int64_t step = 1;
        while (step * D < W) step <<= 1;  // a power of two >= the replicas
        for (step >>= 1; step >= 1; step >>= 1) {
            const int64_t far = step * D;
            const int64_t lim = far < W - far ? far : W - far;
            for (int64_t i = threadIdx.x; i < lim; i += kBlock)
                s_stage[i] = stat_combine<Q>(s_stage[i], s_stage[i + far]);
            __syncthreads();
        }
    }
    double* __restrict__ dst = part + ((int64_t)Q * gridDim.x + blockIdx.x) * nb;
    for (int64_t e = threadIdx.x; e < nb; e += kBlock) dst[e] = s_stage[e];
}

template <typename T>
__global__ void __launch_bounds__(kBlock)
k_colstats_partial(const T* __restrict__ base, int64_t R, int64_t D, int64_t S,
                   int64_t nb, double* __restrict__ part) {
    constexpr int VEC = stat_vec<T>();
    constexpr int U = 4;  // loads in flight per thread
    using V = VecT<T, VEC>;
    __shared__ double s_stage[kBlock * VEC];
    const int64_t N = R * D;
    const int64_t nfull = N / VEC;
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;

    double pv[VEC], acc[4][VEC];
    uint32_t nanf = 0;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        pv[j] = 0.0;
        acc[0][j] = 0.0;
        acc[1][j] = 0.0;
        acc[2][j] = __builtin_inf();
        acc[3][j] = -__builtin_inf();
    }
    auto take = [&](int j, T raw) {
        const double x = stat_f64(raw);
        const double d = x - pv[j];
        acc[0][j] += d;
        acc[1][j] = fma(d, d, acc[1][j]);
        acc[2][j] = fmin(acc[2][j], x);
        acc[3][j] = fmax(acc[3][j], x);
        if constexpr (!std::is_integral_v<T>) nanf |= (x != x) ? (1u << j) : 0u;
    };
    if (t < S) {
        int64_t cc = (t * VEC) % D;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            pv[j] = stat_pivot(base, R, D, cc);
            cc = cc + 1 == D ? 0 : cc + 1;
        }
        const V* __restrict__ vb = reinterpret_cast<const V*>(base);
        int64_t k = t;
        for (; k + (U - 1) * S < nfull; k += U * S) {
            V v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = vb[k + u * S];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < VEC; ++j) take(j, v[u].v[j]);
        }
        for (; k < nfull; k += S) {
            const V v = vb[k];
#pragma unroll
            for (int j = 0; j < VEC; ++j) take(j, v.v[j]);
        }
        if (k == nfull) {  // the last, partial chunk: element loads, in bounds
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                if (nfull * VEC + j < N) take(j, base[nfull * VEC + j]);
        }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j)
        if (nanf & (1u << j)) acc[2][j] = acc[3][j] = __builtin_nan("");
    stat_block_fold<0, VEC>(s_stage, acc[0], D, nb, part);
    stat_block_fold<1, VEC>(s_stage, acc[1], D, nb, part);
    stat_block_fold<2, VEC>(s_stage, acc[2], D, nb, part);
    stat_block_fold<3, VEC>(s_stage, acc[3], D, nb, part);
}

// One column per lane of 32, the blocks of the partial kernel in 8 slices:
// each slice folds its blocks in block order, lane group 0 folds the slices
// in slice order and writes out[0..4][c] = pivot, S1/n (mean = their sum), M2,
// min, max.
constexpr int kStatCols = 32;
constexpr int kStatSlices = kBlock / kStatCols;

template <typename T>
__global__ void __launch_bounds__(kBlock)
k_colstats_final(const T* __restrict__ base, int64_t R, int64_t D,
                 const double* __restrict__ part, int64_t nblocks, int64_t nb,
                 double* __restrict__ out) {
    constexpr int64_t W = (int64_t)kBlock * stat_vec<T>();
    __shared__ double s_red[4][kStatSlices][kStatCols];
    const int cl = threadIdx.x % kStatCols;
    const int sl = threadIdx.x / kStatCols;
    const int64_t c = (int64_t)blockIdx.x * kStatCols + cl;
    double a0 = stat_identity<0>(), a1 = stat_identity<1>(), a2 = stat_identity<2>(),
           a3 = stat_identity<3>();
    if (c < D) {
        const int64_t per = (nblocks + kStatSlices - 1) / kStatSlices;
        const int64_t b0 = sl * per;
        const int64_t b1 = b0 + per < nblocks ? b0 + per : nblocks;
        const int64_t wm = W % D;
        int64_t off = (b0 * wm) % D;  // first column of block b, (b * W) % D
        for (int64_t b = b0; b < b1; ++b) {
            int64_t e = c - off;
            if (e < 0) e += D;
            if (e < nb) {
                a0 = stat_combine<0>(a0, part[(0 * nblocks + b) * nb + e]);
                a1 = stat_combine<1>(a1, part[(1 * nblocks + b) * nb + e]);
                a2 = stat_combine<2>(a2, part[(2 * nblocks + b) * nb + e]);
                a3 = stat_combine<3>(a3, part[(3 * nblocks + b) * nb + e]);
            }
            off += wm;
            if (off >= D) off -= D;
        }
    }
    s_red[0][sl][cl] = a0;
    s_red[1][sl][cl] = a1;
    s_red[2][sl][cl] = a2;
    s_red[3][sl][cl] = a3;
    __syncthreads();
    if (sl == 0 && c < D) {
        for (int s = 1; s < kStatSlices; ++s) {
            a0 = stat_combine<0>(a0, s_red[0][s][cl]);
            a1 = stat_combine<1>(a1, s_red[1][s][cl]);
            a2 = stat_combine<2>(a2, s_red[2][s][cl]);
            a3 = stat_combine<3>(a3, s_red[3][s][cl]);
        }
        // The mean leaves as the pair (pivot, S1/n): the host adds the two
        // only after the cross-rank merge, whose difference of means would
        // otherwise carry the rounding of a large mean into M2.
        const double n = (double)R;
        double m2 = a1 - a0 * (a0 / n);
        if (m2 < 0.0) m2 = 0.0;  // rounding only; a NaN stays
        out[c] = stat_pivot(base, R, D, c);
        out[D + c] = a0 / n;
        out[2 * D + c] = m2;
        out[3 * D + c] = a2;
        out[4 * D + c] = a3;
    }
}

// A/B knobs of the fixed-stride gather, read once (docs/API.md):
//   DDSTORE_GATHER_KERNEL=legacy|tiled  force one kernel family (default:
//                                       by row size, see kTiledMinCpr)
//   DDSTORE_GATHER_BLOCKS=<n>           size of the persistent grid (still
//                                       never more than the work)
//   DDSTORE_GATHER_DIR=lds              LDS directory even at small nparts
//   DDSTORE_GATHER_TILE_ROWS=<n>        cap rows per tile (1..64)
struct GatherKnobs {
    int kernel = 0;  // 0 auto, 1 legacy, 2 tiled
    int blocks = 0;
    bool dir_lds = false;
    int tile_rows = 64;
};
const GatherKnobs& gather_knobs() {
    static const GatherKnobs k = [] {
        GatherKnobs g;
        if (const char* e = getenv("DDSTORE_GATHER_KERNEL")) {
            const std::string s(e);
            g.kernel = s == "legacy" ? 1 : (s == "tiled" ? 2 : 0);
        }
        if (const char* e = getenv("DDSTORE_GATHER_BLOCKS")) {
            const int v = atoi(e);
            if (v > 0) g.blocks = v;
        }
        if (const char* e = getenv("DDSTORE_GATHER_DIR"))
            g.dir_lds = std::string(e) == "lds";
        if (const char* e = getenv("DDSTORE_GATHER_TILE_ROWS")) {
            const int v = atoi(e);
            if (v >= 1 && v <= 64) g.tile_rows = v;
        }
        return g;
    }();
    return k;
}

// CU count of the device the store runs on (one device per process),
// queried once.
int cu_count() {
    static const int n = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) !=
                hipSuccess || v <= 0)
            v = 256;
        return v;
    }();
    return n;
}

// Persistent grid: kBlocksPerCU workgroups of 4 waves per CU (8 = every wave
// slot at occupancy 8), never more than the work. Flagship step time by
// grid on MI355X (256 CUs): 512 blocks 38.99 us, 1024 37.98, 2048 37.65 to
// 38.48 (two run modes), 4096 37.42 -- flat once the wave slots are full.
constexpr int kBlocksPerCU = 8;
// Tiles are sized so that every wave gets about this many when the batch
// allows: fewer leaves wave slots idle, more only shrinks the tile.
constexpr int kTilesPerWave = 2;
// Rows with more chunks than this go to the legacy one-shot mapping: a tile
// is at least one row, and one wave per multi-hundred-KiB row starves the
// chip at small batches.
constexpr int64_t kTiledMaxCpr = 4096;
// Rows with fewer 16-B output chunks than this keep the legacy mapping: a
// tile of <=64 such rows is only a pass or two, so nothing is in flight to
// pay for the tile setup. Measured on MI355X, B=131072, legacy / tiled:
//   f32->f32   64-B rows (4 chunks)   6.05 / 6.44 us
//   u8->f32    16-B rows (4 chunks)   5.81 / 6.43 us
//   f32->bf16 128-B rows (4 chunks)   6.15 / 5.90 us
//   f32->f32  128-B rows (8 chunks)   8.61 / 7.13 us
//   f32->bf16 256-B rows (8 chunks)  11.79 / 10.12 us
constexpr int64_t kTiledMinCpr = 8;

// Launch the tiled core if the shape is eligible; false = caller falls back.
// `re` = elements per row, counted in Tin/Tout elements.
template <typename Tin, typename Tout, typename Xf>
bool launch_tiled(hipStream_t stream, const RowDir& d, const int64_t* idx,
                  int64_t n, int64_t re, Xf xf, Tout* out,
                  unsigned long long* oob) {
    constexpr int VEC = 16 / sizeof(Tout);
    constexpr int INB = VEC * (int)sizeof(Tin);
    constexpr int U = tiled_unroll<INB>();
    const GatherKnobs& kn = gather_knobs();
    if (kn.kernel == 1 || re % VEC != 0 || ((uintptr_t)out % 16) != 0) return false;
    const int64_t cpr = re / VEC;
    if (cpr > kTiledMaxCpr) return false;
    if (kn.kernel != 2 && cpr < kTiledMinCpr) return false;

    int64_t blocks_max = (int64_t)cu_count() * kBlocksPerCU;
    if (kn.blocks > 0) blocks_max = kn.blocks;
    // rows covered by one group of U passes: the smallest useful tile
    int64_t tr_min = (64 * U + cpr - 1) / cpr;
    int64_t tr = n / (blocks_max * (kBlock / 64) * kTilesPerWave);
    if (tr < tr_min) tr = tr_min;
    if (tr > kn.tile_rows) tr = kn.tile_rows;
    const int64_t ntiles = (n + tr - 1) / tr;
    int64_t grid = (ntiles + (kBlock / 64) - 1) / (kBlock / 64);
    if (grid > blocks_max) grid = blocks_max;

    if (d.nparts <= DDS_DIR_KPARTS && !kn.dir_lds) {
        GatherDirK dir;
        const int64_t total = d.h_prefix[d.nparts];
        for (int k = 0; k <= DDS_DIR_KPARTS; ++k)
            dir.prefix[k] = k < d.nparts ? d.h_prefix[k] : total;
        for (int k = 0; k < DDS_DIR_KPARTS; ++k)
            dir.base[k] = k < d.nparts ? d.h_base[k] : nullptr;
        hipLaunchKernelGGL((k_gather_tiled<Tin, Tout, Xf, false>), dim3((unsigned)grid),
                           dim3(kBlock), 0, stream, dir, d.d_base, d.d_prefix, d.nparts,
                           idx, n, ntiles, (uint32_t)cpr, (uint32_t)tr, xf, out, oob);
    } else {
        GatherDirK dir = {};
        hipLaunchKernelGGL((k_gather_tiled<Tin, Tout, Xf, true>), dim3((unsigned)grid),
                           dim3(kBlock), 0, stream, dir, d.d_base, d.d_prefix, d.nparts,
                           idx, n, ntiles, (uint32_t)cpr, (uint32_t)tr, xf, out, oob);
    }
    return true;
}

template <typename Tin, typename Tout, int VEC, typename Xf>
void launch_oneshot(hipStream_t stream, const RowDir& d, const int64_t* idx,
                    int64_t n, int64_t re, Xf xf, Tout* out,
                    unsigned long long* oob) {
    const int grid = n_blocks(n * (re / VEC));
    hipLaunchKernelGGL((k_gather_oneshot<Tin, Tout, VEC, Xf>), dim3(grid), dim3(kBlock),
                       0, stream, d.d_base, d.d_prefix, d.nparts, idx, n, re, xf, out,
                       oob);
}

// Cast and affine gathers: tiled if eligible, else the one-shot kernel with
// 16-B stores if the row and the output pointer allow, else element-wise.
template <typename Tin, typename Tout, typename Xf>
void launch_gather(hipStream_t stream, const RowDir& d, const int64_t* idx,
                   int64_t n, int64_t re, Xf xf, Tout* out,
                   unsigned long long* oob) {
    constexpr int VEC = 16 / sizeof(Tout);
    if (launch_tiled<Tin, Tout>(stream, d, idx, n, re, xf, out, oob)) return;
    if (re % VEC == 0 && ((uintptr_t)out % 16) == 0)
        launch_oneshot<Tin, Tout, VEC>(stream, d, idx, n, re, xf, out, oob);
    else
        launch_oneshot<Tin, Tout, 1>(stream, d, idx, n, re, xf, out, oob);
}

// A type handed to a generic lambda as a value.
template <typename T>
struct TypeTag {
    using type = T;
};

// Calls f(TypeTag<T>{}) with the C++ type of dtype tag `t`; an unknown tag
// calls nothing.
template <typename F>
void dispatch_dtype(int t, F&& f) {
    switch (t) {
        case DDS_U8: f(TypeTag<uint8_t>{}); break;
        case DDS_I32: f(TypeTag<int32_t>{}); break;
        case DDS_I64: f(TypeTag<int64_t>{}); break;
        case DDS_F32: f(TypeTag<float>{}); break;
        case DDS_F64: f(TypeTag<double>{}); break;
        case DDS_F16: f(TypeTag<__half>{}); break;
        case DDS_BF16: f(TypeTag<__hip_bfloat16>{}); break;
        case DDS_F8E4M3: f(TypeTag<__hip_fp8_e4m3>{}); break;
        case DDS_F8E5M2: f(TypeTag<__hip_fp8_e5m2>{}); break;
    }
}

// Calls f(std::integral_constant<int, G>{}) for the listed lane-group size G
// equal to `group`; any other value takes the last one listed.
template <int G0, int... Gs, typename F>
void dispatch_group(int group, F&& f) {
    if constexpr (sizeof...(Gs) == 0) {
        f(std::integral_constant<int, G0>{});
    } else {
        if (group == G0) f(std::integral_constant<int, G0>{});
        else dispatch_group<Gs...>(group, f);
    }
}

} // namespace

void gather_rows(hipStream_t stream, const RowDir& dir,
                 const int64_t* d_idx, int64_t nidx,
                 int64_t row_elems, int in_t, int out_t, const Affine& xf,
                 void* d_out, unsigned long long* d_oob) {
    if (nidx == 0 || row_elems == 0) return;
    const int64_t row_bytes = row_elems * dds_itemsize(in_t);
    // the uint4/VecT paths require a 16/32-B-aligned output pointer; an
    // offset view (e.g. buf[1:]) falls through to the cast/scalar kernels,
    // whose own vector path re-checks alignment
    const uintptr_t out_align = (uintptr_t)d_out;
    if (!xf.on && in_t == out_t && row_bytes % 16 == 0 && out_align % 16 == 0) {
        // NB: a thread-per-row variant (one idx load, all chunks in flight
        // per thread) was measured SLOWER on MI355X for <=64 B rows (7.5 vs
        // 6.1 us at B=131072): fewer, fatter threads lose more to the
        // row-id load+search serialization than they gain in ILP. The
        // chunk-per-thread mapping is used for every row size, with 32-B
        // chunks when the row allows (two dwordx4 loads in flight/thread).
        // A/B on MI355X (B=131072): 512 B rows -- 16B 30.1us / 32B 28.5 /
        // 64B 33.9; 64 B rows -- 16B 6.1 / 32B 6.7 (too few threads per
        // row). 32-B chunks win once a row has >=4 of them.
        // Both experiments above ran on the one-shot grid (per-block
        // prologue, one dependent index load per thread). The tiled core
        // (one index load and owner lookup per ROW, 8 dwordx4 loads in
        // flight per lane, persistent grid) takes rows of >= 8 chunks:
        // B=131072, 512 B rows 28.2 -> 23.3 us, 128 B rows 8.6 -> 7.1 us;
        // 64 B rows stay here (6.05 legacy vs 6.44 tiled).
        if (launch_tiled<uint32_t, uint32_t>(stream, dir, d_idx, nidx, row_bytes / 4,
                                             XfIdentity{}, (uint32_t*)d_out, d_oob))
            return;
        // one 32-B or 16-B vector is the element, so VEC = 1
        using V32 = VecT<uint4, 2>;
        if (row_bytes % 32 == 0 && row_bytes >= 128 && out_align % 32 == 0)
            launch_oneshot<V32, V32, 1>(stream, dir, d_idx, nidx, row_bytes / 32,
                                        XfIdentity{}, (V32*)d_out, d_oob);
        else
            launch_oneshot<uint4, uint4, 1>(stream, dir, d_idx, nidx, row_bytes / 16,
                                            XfIdentity{}, (uint4*)d_out, d_oob);
        return;
    }
    dispatch_dtype(in_t, [&](auto ti) {
        dispatch_dtype(out_t, [&](auto to) {
            using Tin = typename decltype(ti)::type;
            using Tout = typename decltype(to)::type;
            auto launch = [&](auto x) {
                launch_gather<Tin, Tout>(stream, dir, d_idx, nidx, row_elems, x,
                                         (Tout*)d_out, d_oob);
            };
            if (!xf.on) {
                launch(XfCast{});
            } else if constexpr (std::is_same_v<Tout, float> ||
                                 std::is_same_v<Tout, __half> ||
                                 std::is_same_v<Tout, __hip_bfloat16>) {
                // float outputs only
                if (xf.d_scale)
                    launch(XfAffineCol{xf.d_scale, xf.d_shift});
                else
                    launch(XfAffine{xf.scale, xf.shift});
            }
        });
    });
}

void csr_lens(hipStream_t stream, const CsrDir& dir, const int64_t* d_idx,
              int64_t nidx, int64_t* d_lens,
              unsigned long long* d_oob, unsigned long long* d_elems) {
    if (nidx == 0) return;
    hipLaunchKernelGGL(k_csr_lens, dim3(n_blocks(nidx)), dim3(kBlock), 0, stream,
                       dir.d_goff, d_idx, nidx, dir.nsamples_total, d_lens, d_oob,
                       d_elems);
}

void gather_csr(hipStream_t stream, const CsrDir& dir,
                const int64_t* d_idx, int64_t nidx,
                const int64_t* d_out_off,
                int64_t elem_bytes, int64_t cap_elems,
                void* d_out, unsigned long long* d_ctrs) {
    if (nidx == 0) return;
    // lanes cooperating per sample: small groups amortize the per-sample
    // setup (row-id load + directory search) across the wave and keep more
    // samples in flight. A/B on MI355X: GROUP=16 wins or ties from 512 B to
    // 32 KiB average samples (2.23 vs 1.44 G samples/s at 512 B vs GROUP=64)
    // -- the only reason to grow the group is chip COVERAGE when the batch
    // has few samples (need >=1024 workgroups across 256 CUs).
    static const int g_override = [] {
        const char* e = getenv("DDSTORE_CSR_GROUP");
        return e ? atoi(e) : 0;
    }();
    int group = nidx >= 16384 ? 16 : (nidx >= 4096 ? 64 : 256);
    if (g_override) group = g_override;
    int64_t b = (nidx + (kBlock / group) - 1) / (kBlock / group);
    const int grid = (int)(b < kMaxBlocks ? b : kMaxBlocks);
    // vector paths reinterpret d_out; a misaligned output (e.g. an offset
    // view) falls back to the next-narrower granularity
    const uintptr_t oa = (uintptr_t)d_out;
    auto launch = [&](auto unit) {
        using U = typename decltype(unit)::type;
        dispatch_group<8, 16, 32, 64, 256>(group, [&](auto G) {
            hipLaunchKernelGGL((k_gather_csr_wave<U, G()>), dim3(grid), dim3(kBlock), 0,
                               stream, dir.d_base, dir.d_sample_prefix,
                               dir.d_elem_prefix, dir.nparts, dir.d_goff, d_idx, nidx,
                               d_out_off, elem_bytes / (int64_t)sizeof(U), cap_elems,
                               (U*)d_out, d_ctrs);
        });
    };
    if (elem_bytes % 16 == 0 && oa % 16 == 0) {
        launch(TypeTag<uint4>{});
    } else if (elem_bytes % 4 == 0 && oa % 4 == 0) {
        // 4/8-B-granular elements: dword addressing, stores re-aligned to
        // dwordx4 inside each sample's payload
        launch(TypeTag<uint32_t>{});
    } else {
        launch(TypeTag<uint8_t>{});
    }
}

void gather_csr_padded(hipStream_t stream, const CsrDir& dir,
                       const int64_t* d_idx, int64_t nidx,
                       int64_t row_elems, int64_t max_len, int in_t, int out_t,
                       const Affine& xf, uint64_t pad_bits,
                       void* d_out, int64_t* d_lengths,
                       unsigned long long* d_ctrs) {
    if (nidx == 0) return;
    if (row_elems == 0 || max_len == 0) {
        // no payload to move: lengths and the bad-index count only
        csr_lens(stream, dir, d_idx, nidx, d_lengths, d_ctrs + DDS_CTR_OOB, nullptr);
        return;
    }
    // the pad's raw bits, replicated over one 16-B output chunk
    const int osz = dds_itemsize(out_t);
    unsigned char pb[16];
    for (int i = 0; i < 16; ++i) pb[i] = (unsigned char)(pad_bits >> (8 * (i % osz)));
    dds_u32x4 pad16;
    __builtin_memcpy(&pad16, pb, 16);
    const uintptr_t oa = (uintptr_t)d_out;
    // `disp` counts Tin/Tout units per element
    auto launch = [&](auto ti, auto to, auto vec, auto x, int64_t disp, bool aligned) {
        using Tin = typename decltype(ti)::type;
        using Tout = typename decltype(to)::type;
        constexpr int VEC = decltype(vec)::value;
        // lanes per row: the chunks of one row, 8..64; the whole block for
        // few long rows (chip coverage, as in gather_csr)
        const int64_t cpr = max_len * disp / VEC;
        int lg = cpr <= 8 ? 3 : (cpr <= 16 ? 4 : (cpr <= 32 ? 5 : 6));
        if (cpr > 64 && nidx < 4096) lg = 8;
        const int64_t gpb = kBlock >> lg;
        const int64_t b = (nidx + gpb - 1) / gpb;
        hipLaunchKernelGGL((k_gather_csr_padded<Tin, Tout, VEC, decltype(x)>),
                           dim3((unsigned)(b < kMaxBlocks ? b : kMaxBlocks)),
                           dim3(kBlock), 0, stream, dir.d_base, dir.d_sample_prefix,
                           dir.d_elem_prefix, dir.nparts, dir.d_goff, d_idx, nidx, disp,
                           max_len, lg, aligned, x, pad16, (Tout*)d_out, d_lengths,
                           d_ctrs);
    };
    const int64_t elem_bytes = row_elems * dds_itemsize(in_t);
    if (!xf.on && in_t == out_t && elem_bytes % 16 == 0 && oa % 16 == 0) {
        // byte move: one uint4 is the unit, so VEC = 1
        launch(TypeTag<uint4>{}, TypeTag<uint4>{}, std::integral_constant<int, 1>{},
               XfIdentity{}, elem_bytes / 16, true);
        return;
    }
    // 16-B stores if the output pointer and the row allow (vector loads if
    // the element width allows as well), else element-wise
    auto launch_xf = [&](auto ti, auto to, auto x) {
        using Tout = typename decltype(to)::type;
        constexpr int VEC = 16 / sizeof(Tout);
        if (oa % 16 == 0 && (max_len * row_elems) % VEC == 0)
            launch(ti, to, std::integral_constant<int, VEC>{}, x, row_elems,
                   row_elems % VEC == 0);
        else
            launch(ti, to, std::integral_constant<int, 1>{}, x, row_elems, true);
    };
    dispatch_dtype(in_t, [&](auto ti) {
        dispatch_dtype(out_t, [&](auto to) {
            using Tout = typename decltype(to)::type;
            if (!xf.on) {
                launch_xf(ti, to, XfCast{});
            } else if constexpr (std::is_same_v<Tout, float> ||
                                 std::is_same_v<Tout, __half> ||
                                 std::is_same_v<Tout, __hip_bfloat16>) {
                // float outputs only
                if (xf.d_scale)
                    launch_xf(ti, to, XfAffineCol{xf.d_scale, xf.d_shift});
                else
                    launch_xf(ti, to, XfAffine{xf.scale, xf.shift});
            }
        });
    });
}

// ---- column statistics (kernels: k_colstats_partial / k_colstats_final) ----
namespace {
struct StatPlan {
    int64_t blocks, S, nb;
};
// The grid of the partial kernel. Scratch formula: blocks * nb partial
// entries of 4 doubles (S1, S2, min, max), nb = min(D, 256 * VEC) -- a
// function of D and the grid only, never of the number of rows.
StatPlan stat_plan(int64_t rows, int64_t D, int in_t) {
    const int isz = dds_itemsize(in_t);
    const int64_t vec = isz == 1 ? 8 : 16 / isz;
    int64_t g = D, h = vec;  // gcd(D, vec)
    while (h) {
        const int64_t r = g % h;
        g = h;
        h = r;
    }
    const int64_t dp = D / g;  // S is a multiple of this
    const int64_t nchunks = (rows * D + vec - 1) / vec;
    // >= 32 chunks per thread before the grid grows, 4 blocks per CU at most
    int64_t b = nchunks / ((int64_t)kBlock * 32);
    const int64_t target = (int64_t)cu_count() * 4;
    if (b > target) b = target;
    if (b < 1) b = 1;
    const int64_t need = (dp + kBlock - 1) / kBlock;  // every column has a thread
    if (b < need) b = need;
    const int64_t W = (int64_t)kBlock * vec;
    return StatPlan{b, (b * kBlock / dp) * dp, D < W ? D : W};
}
}  // namespace

size_t colstats_scratch_bytes(int64_t rows, int64_t row_elems, int in_t) {
    if (rows <= 0 || row_elems <= 0) return 0;
    const StatPlan p = stat_plan(rows, row_elems, in_t);
    return (size_t)(p.blocks * p.nb * 4) * sizeof(double);
}

void column_stats(hipStream_t stream, const void* d_base, int64_t rows,
                  int64_t row_elems, int in_t, void* d_scratch, double* d_out) {
    if (rows <= 0 || row_elems <= 0) return;
    const StatPlan p = stat_plan(rows, row_elems, in_t);
    const int64_t fb = (row_elems + kStatCols - 1) / kStatCols;
    dispatch_dtype(in_t, [&](auto ti) {
        using T = typename decltype(ti)::type;
        hipLaunchKernelGGL((k_colstats_partial<T>), dim3((unsigned)p.blocks),
                           dim3(kBlock), 0, stream, (const T*)d_base, rows, row_elems,
                           p.S, p.nb, (double*)d_scratch);
        hipLaunchKernelGGL((k_colstats_final<T>), dim3((unsigned)fb), dim3(kBlock), 0,
                           stream, (const T*)d_base, rows, row_elems,
                           (const double*)d_scratch, p.blocks, p.nb, d_out);
    });
}

size_t csr_plan_scratch_bytes(int64_t nidx) {
    const int64_t ntiles = (nidx + kBlock - 1) / kBlock;
    return (size_t)(2 * (ntiles > 0 ? ntiles : 1) + 2 * (nidx > 0 ? nidx : 1)
                    + 2) * sizeof(int64_t);
}

int64_t csr_item_elems(int64_t elem_bytes) {
    static const int item_bytes = [] {
        const char* e = getenv("DDSTORE_CSR_ITEM");
        int v = e ? atoi(e) : kItemBytes;
        return v >= 16 ? v : kItemBytes;
    }();
    int64_t ie = item_bytes / (elem_bytes > 0 ? elem_bytes : 1);
    return ie > 0 ? ie : 1;
}

void gather_csr_balanced(hipStream_t stream, const CsrDir& dir,
                         const int64_t* d_idx, int64_t nidx,
                         int64_t elem_bytes, int64_t cap_elems,
                         int64_t* d_out_off, void* d_out,
                         unsigned long long* d_ctrs,
                         void* d_scratch, int64_t* d_desc, int64_t desc_cap) {
    if (nidx == 0) return;
    const int64_t ntiles = (nidx + kBlock - 1) / kBlock;
    int64_t* aggs = reinterpret_cast<int64_t*>(d_scratch);
    int64_t* lens_tmp = aggs + 2 * ntiles;
    int64_t* e0_tmp = lens_tmp + nidx;
    int64_t* meta = e0_tmp + nidx;
    const int64_t item_elems = csr_item_elems(elem_bytes);
    const uintptr_t oa = (uintptr_t)d_out;
    const bool dw = elem_bytes % 4 == 0 && oa % 4 == 0;
    const int64_t upe = dw ? elem_bytes / 4 : elem_bytes;  // units per elem
    const int g1 = (int)(ntiles < kMaxBlocks ? ntiles : kMaxBlocks);
    hipLaunchKernelGGL(k_csr_plan1, dim3(g1), dim3(kBlock), 0, stream, dir.d_goff,
                       dir.nsamples_total, d_idx, nidx, item_elems, lens_tmp,
                       e0_tmp, aggs, d_ctrs);
    hipLaunchKernelGGL(k_csr_plan2, dim3(1), dim3(kBlock), 0, stream, aggs,
                       ntiles, meta, d_ctrs);
    hipLaunchKernelGGL(k_csr_plan3, dim3(g1), dim3(kBlock), 0, stream,
                       lens_tmp, e0_tmp, nidx, dir.d_sample_prefix, dir.d_elem_prefix,
                       dir.nparts, d_idx, item_elems, upe, cap_elems, aggs,
                       d_out_off, d_desc, desc_cap, d_ctrs);
    static const int item_group = [] {
        const char* e = getenv("DDSTORE_CSR_ITEM_GROUP");
        int v = e ? atoi(e) : 16;
        return (v == 8 || v == 16 || v == 32) ? v : 16;
    }();
    const int64_t gi = (desc_cap + (kBlock / item_group) - 1)
                       / (kBlock / item_group);
    const int g2 = (int)(gi < kMaxBlocks ? gi : kMaxBlocks);
    auto launch = [&](auto unit, auto G) {
        using U = typename decltype(unit)::type;
        hipLaunchKernelGGL((k_gather_csr_items<U, G()>), dim3(g2), dim3(kBlock), 0,
                           stream, dir.d_base, dir.nparts, d_desc, meta, desc_cap,
                           (U*)d_out);
    };
    if (dw) {
        dispatch_group<8, 32, 16>(item_group, [&](auto G) {
            launch(TypeTag<uint32_t>{}, G);
        });
    } else {
        launch(TypeTag<uint8_t>{}, std::integral_constant<int, 16>{});
    }
}

void csr_offsets(hipStream_t stream, const CsrDir& dir,
                 const int64_t* d_idx, int64_t nidx, int64_t* d_out_off,
                 void* d_scratch, unsigned long long* d_ctrs) {
    if (nidx == 0) return;
    const int64_t ntiles = (nidx + kBlock - 1) / kBlock;
    int64_t* aggs = reinterpret_cast<int64_t*>(d_scratch);
    int64_t* lens_tmp = aggs + 2 * ntiles;
    int64_t* e0_tmp = lens_tmp + nidx;
    int64_t* meta = e0_tmp + nidx;
    const int g1 = (int)(ntiles < kMaxBlocks ? ntiles : kMaxBlocks);
    // no work items here: one element per item keeps plan1's item count finite
    hipLaunchKernelGGL(k_csr_plan1, dim3(g1), dim3(kBlock), 0, stream, dir.d_goff,
                       dir.nsamples_total, d_idx, nidx, (int64_t)1, lens_tmp, e0_tmp,
                       aggs, d_ctrs);
    hipLaunchKernelGGL(k_csr_plan2, dim3(1), dim3(kBlock), 0, stream, aggs,
                       ntiles, meta, d_ctrs);
    hipLaunchKernelGGL(k_csr_scan3, dim3(g1), dim3(kBlock), 0, stream, lens_tmp,
                       nidx, aggs, d_out_off);
}

void gather_csr_relabel(hipStream_t stream, const CsrDir& dir,
                        const int64_t* d_idx, int64_t nidx,
                        const int64_t* d_ptr, const int64_t* d_edge_ptr,
                        int64_t ncap, int64_t ecap, int in_t, int out_t, bool coo,
                        void* d_out, unsigned long long* d_ctrs) {
    if (nidx == 0) return;  // ecap == 0 still counts the dropped graphs
    constexpr int G = kGraphGroup;
    const int64_t b = (nidx + (kBlock / G) - 1) / (kBlock / G);
    const int grid = (int)(b < kMaxBlocks ? b : kMaxBlocks);
    auto launch = [&](auto ti, auto to, auto c) {
        using Tin = typename decltype(ti)::type;
        using Tout = typename decltype(to)::type;
        hipLaunchKernelGGL((k_gather_csr_relabel<Tin, Tout, G, decltype(c)::value>),
                           dim3(grid), dim3(kBlock), 0, stream, dir.d_base,
                           dir.d_sample_prefix, dir.d_elem_prefix, dir.nparts,
                           dir.d_goff, d_idx, nidx, d_ptr, d_edge_ptr, ncap, ecap,
                           (Tout*)d_out, d_ctrs);
    };
    auto launch_coo = [&](auto ti, auto to) {
        if (coo) launch(ti, to, std::true_type{});
        else launch(ti, to, std::false_type{});
    };
    // the three id widenings: i64 -> i64, i32 -> i64, i32 -> i32 (the host
    // refuses everything else)
    if (in_t == DDS_I64 && out_t == DDS_I64)
        launch_coo(TypeTag<int64_t>{}, TypeTag<int64_t>{});
    else if (in_t == DDS_I32 && out_t == DDS_I64)
        launch_coo(TypeTag<int32_t>{}, TypeTag<int64_t>{});
    else if (in_t == DDS_I32 && out_t == DDS_I32)
        launch_coo(TypeTag<int32_t>{}, TypeTag<int32_t>{});
}

void graph_fill(hipStream_t stream, const int64_t* d_ptr, const int64_t* d_edge_ptr,
                int64_t nidx, int64_t ncap, int64_t ecap, int out_t, bool coo,
                int64_t edge_fill, int64_t* d_batch, void* d_edge_out) {
    if (ncap == 0 && ecap == 0) return;
    constexpr int G = kGraphGroup;
    // one thread per 64 B of output, or one group per graph if that is more
    const int64_t by_graph = (nidx + (kBlock / G) - 1) / (kBlock / G);
    const int64_t by_bytes =
        (ncap * 8 + 2 * ecap * (int64_t)dds_itemsize(out_t)) / (64 * kBlock) + 1;
    const int64_t b = by_graph > by_bytes ? by_graph : by_bytes;
    const int grid = (int)(b < kMaxBlocks ? b : kMaxBlocks);
    if (out_t == DDS_I64)
        hipLaunchKernelGGL((k_graph_fill<int64_t, G>), dim3(grid), dim3(kBlock), 0,
                           stream, d_ptr, d_edge_ptr, nidx, ncap, ecap, coo,
                           edge_fill, d_batch, (int64_t*)d_edge_out);
    else if (out_t == DDS_I32)
        hipLaunchKernelGGL((k_graph_fill<int32_t, G>), dim3(grid), dim3(kBlock), 0,
                           stream, d_ptr, d_edge_ptr, nidx, ncap, ecap, coo,
                           (int32_t)edge_fill, d_batch, (int32_t*)d_edge_out);
}

void scatter_rows_local(hipStream_t stream,
                        void* d_base, int64_t nrows_local,
                        int64_t row_elems, int elem_t,
                        const int64_t* d_local_idx, int64_t nidx,
                        const void* d_src, unsigned long long* d_oob) {
    if (nidx == 0 || row_elems == 0) return;
    const int64_t row_bytes = row_elems * dds_itemsize(elem_t);
    const uintptr_t al = (uintptr_t)d_src | (uintptr_t)d_base;
    auto launch = [&](auto chunk) {
        using V = typename decltype(chunk)::type;
        const int64_t cpr = row_bytes / (int64_t)sizeof(V);
        hipLaunchKernelGGL((k_scatter_rows<V>), dim3(n_blocks(nidx * cpr)),
                           dim3(kBlock), 0, stream, (V*)d_base, nrows_local, cpr,
                           d_local_idx, nidx, (const V*)d_src, d_oob);
    };
    if (row_bytes % 32 == 0 && row_bytes >= 128 && al % 32 == 0)
        launch(TypeTag<VecT<uint4, 2>>{});
    else if (row_bytes % 16 == 0 && al % 16 == 0)
        launch(TypeTag<uint4>{});
    else
        launch(TypeTag<uint8_t>{});
}

} // namespace ddstore
