// ddstore_amd kernel launcher declarations (host-side interface).
//
// MI355X-native hot path of the store: the reference performs one synchronous
// MPI_Get / fi_read per row (reference: include/ddstore.hpp:229-237,
// src/common.cxx:332-343); here a whole minibatch of rows is gathered by ONE
// kernel launch that reads local + xGMI-peer HBM pointers directly and packs
// (optionally dtype-casting) into a contiguous output buffer.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

// Element dtype enum shared between host dispatch and kernels.
// bool is stored/moved as u8 (values 0/1), matching NumPy's memory layout.
enum DDSType : int {
    DDS_U8 = 0,
    DDS_I32 = 1,
    DDS_I64 = 2,
    DDS_F32 = 3,
    DDS_F64 = 4,
    DDS_F16 = 5,
    DDS_BF16 = 6,
    DDS_F8E4M3 = 7,   // OCP e4m3fn (gfx950-native fp8, NOT MI300X fnuz)
    DDS_F8E5M2 = 8,
    DDS_NUM_TYPES = 9
};

// Max world size the in-kernel directory supports (fits in LDS; one node of
// 8 GPUs is the design point, 128 leaves headroom for oversubscribed tests).
#define DDS_MAX_PARTS 128

// Per-variable device counter block layout (unsigned long long[DDS_NCTR]):
//   [0] oob_skipped  -- out-of-range sample indices skipped by a gather
//   [1] cap_skipped  -- CSR samples skipped because the output capacity
//                       buffer was too small (never write past it)
//   [2] csr_elems    -- true elements gathered by gather_csr_fast (stats;
//                       the capacity-buffer size would over-report)
#define DDS_CTR_OOB 0
#define DDS_CTR_CAP 1
#define DDS_CTR_ELEMS 2
#define DDS_NCTR 3

// Worlds up to this size (one node, the design point) get the owner
// directory BY VALUE in the gather kernel's arguments; larger ones stage the
// device copy in LDS.
#define DDS_DIR_KPARTS 8

namespace ddstore {

// Kernel-argument form of the directory. The host pads prefix[k] for
// k >= nparts with the total row count (so prefix[DDS_DIR_KPARTS] is always
// the total and owner lookup needs no nparts) and base[k] with nullptr.
struct GatherDirK {
    int64_t prefix[DDS_DIR_KPARTS + 1];
    const void* base[DDS_DIR_KPARTS];
};

// Element size in bytes of a DDSType tag.
inline int64_t dds_itemsize(int t) {
    switch (t) {
        case DDS_U8: case DDS_F8E4M3: case DDS_F8E5M2: return 1;
        case DDS_F16: case DDS_BF16: return 2;
        case DDS_I32: case DDS_F32: return 4;
        default: return 8;
    }
}

// Owner directory of a fixed-stride variable, in both copies:
//   d_base   : device array[nparts]   -- shard base pointers (self + IPC peers)
//   d_prefix : device array[nparts+1] -- global row prefix sums, prefix[0]=0
//   h_base   : HOST copy of d_base (array[nparts])
//   h_prefix : HOST copy of d_prefix (array[nparts+1])
// The host copies feed the kernel-argument directory of the tiled kernel
// (nparts <= DDS_DIR_KPARTS); the device copies serve the LDS-staged
// variant and the scalar fallbacks. Both must describe the same shards.
struct RowDir {
    const void* const* d_base;
    const int64_t* d_prefix;
    const void* const* h_base;
    const int64_t* h_prefix;
    int nparts;
};

// Owner directory of a CSR variable (device memory throughout): sample `g`
// owns elements [d_goff[g], d_goff[g+1]) of the global element space.
//   d_base          : array[nparts]   -- shard base pointers
//   d_sample_prefix : array[nparts+1] -- per-rank sample-count prefix sums
//   d_elem_prefix   : array[nparts+1] -- per-rank element-count prefix sums
//   d_goff          : array[nsamples_total+1] -- replicated element offsets
struct CsrDir {
    const void* const* d_base;
    const int64_t* d_sample_prefix;
    const int64_t* d_elem_prefix;
    int nparts;
    const int64_t* d_goff;
    int64_t nsamples_total;
};

// What a fetch does to each element on the way. !on: byte move if the
// dtypes agree, else a numeric cast. on: out = cast(in) * scale + shift (f32
// math; float output dtypes only) -- data-loader normalization folded into
// the fetch. With d_scale != nullptr the pair is per column instead:
// out[r][c] = cast(in[r][c]) * d_scale[c] + d_shift[c], same rounding
// contract; d_scale and d_shift are device arrays of row_elems floats each,
// 16-B aligned, on the store device, and `scale` / `shift` are unused.
struct Affine {
    bool on = false;
    float scale = 1.0f, shift = 0.0f;
    const float* d_scale = nullptr;
    const float* d_shift = nullptr;
};

// Gather `nidx` fixed-stride rows (row = `row_elems` elements of dtype
// `in_t`) addressed by global row ids `d_idx` from the sharded store
// described by `dir`, packing them contiguously into `d_out` with dtype
// `out_t` through `xf`.
// d_oob: device counter incremented once per out-of-range index (the row is
// skipped instead of read out of bounds; checked lazily via query()).
void gather_rows(hipStream_t stream, const RowDir& dir,
                 const int64_t* d_idx, int64_t nidx,
                 int64_t row_elems, int in_t, int out_t, const Affine& xf,
                 void* d_out, unsigned long long* d_oob);

// CSR (variable-length record) gather: each element is `elem_bytes` bytes
// (= disp * itemsize). Output element offsets per sample are provided in
// d_out_off (exclusive scan, [nidx+1]). `cap_elems` is the
// output buffer's capacity in elements: a non-empty sample whose slice would
// end past it is SKIPPED and counted in d_ctrs[DDS_CTR_CAP] (never written
// OOB). An empty sample writes nothing and is never counted.
void gather_csr(hipStream_t stream, const CsrDir& dir,
                const int64_t* d_idx, int64_t nidx,
                const int64_t* d_out_off,
                int64_t elem_bytes, int64_t cap_elems,
                void* d_out, unsigned long long* d_ctrs);

// lens[i] = goff[idx[i]+1] - goff[idx[i]] (CSR gather plan helper; reads
// dir.d_goff and dir.nsamples_total only). If d_elems != nullptr the true
// total (sum of lens) is accumulated into it (wave-reduced; used by
// gather_csr_fast for exact byte stats).
void csr_lens(hipStream_t stream, const CsrDir& dir, const int64_t* d_idx,
              int64_t nidx, int64_t* d_lens,
              unsigned long long* d_oob, unsigned long long* d_elems);

// Balanced one-call CSR fetch: three tiny plan kernels (per-tile lens+scan,
// single-block tile-aggregate scan, finalize + work-item emission) followed
// by an item-parallel gather. Samples are split into <=1024-B work items so
// gather waves get near-uniform work (the per-sample kernel loses ~1.5x to
// max-of-N-samples-per-wave imbalance; r2 fixed-len A/B). Writes
// d_out_off[nidx+1]; accumulates true gathered elements into
// d_ctrs[DDS_CTR_ELEMS]. A sample with L > 0 elements whose slice would end
// past cap_elems is skipped: nothing of it is written, it counts once in
// d_ctrs[DDS_CTR_CAP], and d_out_off still carries the unclamped scan. A
// zero-length sample writes nothing and is never counted.
// d_scratch: csr_plan_scratch_bytes(nidx) bytes (no zeroing needed);
// d_desc: desc_cap work-item descriptors of 2 int64 each, desc_cap =
// cap_elems / csr_item_elems(elem_bytes) + nidx, no zeroing needed either:
// the gather acts only on slots below min(item total, desc_cap), and the plan
// writes every one of them in the same call (zero-length for the slots of
// skipped samples), whatever the buffer held before.
size_t csr_plan_scratch_bytes(int64_t nidx);
int64_t csr_item_elems(int64_t elem_bytes);
void gather_csr_balanced(hipStream_t stream, const CsrDir& dir,
                         const int64_t* d_idx, int64_t nidx,
                         int64_t elem_bytes, int64_t cap_elems,
                         int64_t* d_out_off, void* d_out,
                         unsigned long long* d_ctrs,
                         void* d_scratch, int64_t* d_desc, int64_t desc_cap);

// Padded CSR gather, ONE launch: sample d_idx[s] is written to row s of a
// dense (nidx, max_len, row_elems) output of dtype `out_t` -- its first
// min(len, max_len) elements through the byte move / cast / affine `xf`
// (f32/f16/bf16 outputs only when xf.on; a column of the per-column form is
// an element's flat position in [0, row_elems)), the rest of the row filled
// with the pad. `pad_bits` holds the raw bits of ONE output element in its
// low bytes; the kernel broadcasts them and applies neither cast nor affine
// to them. d_lengths[s] receives the true stored length (not clipped to
// max_len). An out-of-range index gives an all-pad row, length 0, and one
// count in d_ctrs[DDS_CTR_OOB]. The true gathered elements, sum(min(len,
// max_len)), accumulate into d_ctrs[DDS_CTR_ELEMS]. Every output element is
// written exactly once; no scratch, no host reads of device data.
void gather_csr_padded(hipStream_t stream, const CsrDir& dir,
                       const int64_t* d_idx, int64_t nidx,
                       int64_t row_elems, int64_t max_len, int in_t, int out_t,
                       const Affine& xf, uint64_t pad_bits,
                       void* d_out, int64_t* d_lengths,
                       unsigned long long* d_ctrs);

// Column statistics of one local shard, viewed as a row-major (rows,
// row_elems) array of dtype `in_t` (for a CSR variable: its elements). Writes
// d_out[0..5*row_elems): for every column, as f64, a pivot p taken from its
// values and the offset o with mean = p + o (kept apart so that a merge with
// another shard's result can difference the means without the rounding of a
// large mean), M2 = sum((x - mean)^2), min and max; a column with a NaN has
// NaN in o, M2, min and max. Two kernels on
// `stream`, deterministic (no atomics), reads only [d_base, d_base + rows *
// row_elems). d_scratch: colstats_scratch_bytes(...) bytes, no zeroing
// needed; its size depends on row_elems and the grid, not on `rows`.
// rows == 0 or row_elems == 0 launches nothing and writes nothing.
size_t colstats_scratch_bytes(int64_t rows, int64_t row_elems, int in_t);
void column_stats(hipStream_t stream, const void* d_base, int64_t rows,
                  int64_t row_elems, int in_t, void* d_scratch, double* d_out);

// Graph-batch fetch (DeviceStore::gather_graph): the pieces beside the node
// features, which gather_csr_balanced fetches unchanged.
//
// csr_offsets: d_out_off[0..nidx] = exclusive scan of the requested samples'
// lengths (a bad index has length 0), never clamped. It runs k_csr_plan1 and
// k_csr_plan2 as they are, so bad indices count in d_ctrs[DDS_CTR_OOB] and the
// requested total is ADDED to d_ctrs[DDS_CTR_ELEMS]: the gather that follows
// takes back what it drops. d_scratch: csr_plan_scratch_bytes(nidx) bytes.
void csr_offsets(hipStream_t stream, const CsrDir& dir,
                 const int64_t* d_idx, int64_t nidx, int64_t* d_out_off,
                 void* d_scratch, unsigned long long* d_ctrs);

// Relabelling gather of an edge-index variable (2 ids per element, in_t
// DDS_I32 or DDS_I64; out_t DDS_I64, or DDS_I32 for DDS_I32 input). d_ptr and
// d_edge_ptr are the [nidx+1] node and edge offsets of the request. The edges
// of graph s are written iff d_ptr[s+1] <= ncap and d_edge_ptr[s+1] <= ecap:
// id + d_ptr[s], edge e at column d_edge_ptr[s] + e of a (2, ecap) output
// (coo) or at that row of an (ecap, 2) output. A graph with edges that are
// not written counts once in d_ctrs[DDS_CTR_CAP] and its edges are subtracted
// from d_ctrs[DDS_CTR_ELEMS]. Slots of no kept edge are left to graph_fill.
void gather_csr_relabel(hipStream_t stream, const CsrDir& dir,
                        const int64_t* d_idx, int64_t nidx,
                        const int64_t* d_ptr, const int64_t* d_edge_ptr,
                        int64_t ncap, int64_t ecap, int in_t, int out_t, bool coo,
                        void* d_out, unsigned long long* d_ctrs);

// The rest of a graph batch, one launch, no atomics: d_batch[j] = s for the
// nodes of every graph with d_ptr[s+1] <= ncap and nidx for the slots behind
// them up to ncap; every edge_index slot behind the kept edges (the graphs
// gather_csr_relabel writes) up to ecap = edge_fill. Together with
// gather_csr_relabel every element of both buffers is written exactly once.
// d_ptr / d_edge_ptr must hold nidx + 1 entries (one zero for nidx == 0).
void graph_fill(hipStream_t stream, const int64_t* d_ptr, const int64_t* d_edge_ptr,
                int64_t nidx, int64_t ncap, int64_t ecap, int out_t, bool coo,
                int64_t edge_fill, int64_t* d_batch, void* d_edge_out);

// Scatter rows of a packed buffer into the local shard at arbitrary local row
// ids (inverse of gather_rows with nparts==1). Used by the epoch reshuffle to
// place all-to-all-received rows.
void scatter_rows_local(hipStream_t stream,
                        void* d_base, int64_t nrows_local,
                        int64_t row_elems, int elem_t,
                        const int64_t* d_local_idx, int64_t nidx,
                        const void* d_src, unsigned long long* d_oob);

} // namespace ddstore
