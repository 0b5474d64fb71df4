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

// Radius-graph fetch (DeviceStore::gather_radius_graph): the edges of a batch
// of graphs built from their node positions. d_pos holds the packed positions
// of the request, (ncap, 3) of pos_t (DDS_F32 or DDS_F64; anything else
// launches nothing), as gather_csr_balanced has just written them on the same
// stream, and d_ptr its [nidx+1] offsets: local, contiguous memory, so neither
// launcher needs an owner directory. Each coordinate is taken as f32 (f64
// rounds to nearest even); for nodes i, j of one graph d = pos[i] - pos[j] per
// coordinate, d2 = (dx*dx + dy*dy) + dz*dz in f32 without contraction, and
// (src = i, dst = j) is an edge iff d2 <= r2 and (i != j or loop). A graph's
// edges are ordered by dst, then src; with max_neighbors = K > 0 every dst
// keeps its first K sources in that order (K <= 0: all).
//
// radius_count: d_edge_ptr[0..nidx] = exclusive scan of the per-graph edge
// counts, where a graph with d_ptr[s+1] > ncap (its positions were not
// fetched) and an empty one count 0; never clamped by any edge capacity. It
// leaves the per-node degrees in d_scratch for radius_fill. Two launches.
// d_scratch: radius_scratch_bytes(nidx, ncap) bytes, no zeroing needed.
//
// radius_fill: the edges of every graph with d_ptr[s+1] <= ncap and
// d_edge_ptr[s+1] <= ecap, edge e at column d_edge_ptr[s] + e of a (2, ecap)
// output of out_t (DDS_I64 or DDS_I32; coo) or at that row of an (ecap, 2)
// one, both ids shifted by d_ptr[s]; with d_vec_out != nullptr row
// d_edge_ptr[s] + e of that (ecap, 3) f32 array is (dx, dy, dz). d_scratch and
// every other argument are radius_count's, on the same stream. Slots of no
// kept edge are left to graph_fill (edge index) or untouched (vectors). One
// launch; no atomics and no counters in either.
//
// radius_tile_nodes: the nodes one LDS slice holds; larger graphs stream
// through it (a second code path, for tests to aim at).
//
// Nearest mode (docs/API.md): with k in 1..radius_nearest_max() every dst
// keeps its min(k, degree) edges of smallest key (d2 bits, src), still ordered
// by src. radius_nearest_select stands for radius_count (same outputs; it
// also leaves a threshold key per node in d_scratch; k out of range launches
// nothing) and radius_fill takes nearest = true; both need
// radius_scratch_bytes(nidx, ncap, true) bytes, 12 per node.
int radius_tile_nodes();
int radius_nearest_max();
size_t radius_scratch_bytes(int64_t nidx, int64_t ncap, bool nearest = false);
void radius_nearest_select(hipStream_t stream, const void* d_pos, int pos_t,
                           const int64_t* d_ptr, int64_t nidx, int64_t ncap, float r2,
                           int k, bool loop, void* d_scratch, int64_t* d_edge_ptr);
void radius_count(hipStream_t stream, const void* d_pos, int pos_t,
                  const int64_t* d_ptr, int64_t nidx, int64_t ncap, float r2,
                  int64_t max_neighbors, bool loop, void* d_scratch,
                  int64_t* d_edge_ptr);
void radius_fill(hipStream_t stream, const void* d_pos, int pos_t,
                 const int64_t* d_ptr, const int64_t* d_edge_ptr, int64_t nidx,
                 int64_t ncap, int64_t ecap, float r2, bool loop,
                 const void* d_scratch, int out_t, bool coo, void* d_edge_out,
                 float* d_vec_out, bool nearest = false);

// Cell-list path of the same fetch (docs/API.md, algorithm = "cells"): the
// same rule, order and outputs bit for bit, found through a spatial grid per
// graph in O(nodes), every graph spread over the whole device. The launchers
// take r itself (the bin width comes from it; r2 = r * r in f32 as above).
//
// radius_cells_count stands for radius_count: d_edge_ptr as it leaves it, and
// in d_scratch the nodes in bin order, the grids and every node's first edge
// slot for radius_cells_fill. d_scratch: radius_cells_scratch_bytes(nidx,
// ncap) bytes, under 112 * (ncap + nidx) + 256 whatever the coordinates are,
// 16-byte aligned, no zeroing needed. Needs ncap + nidx < 2^31, which the
// caller checks. Integer atomics place the nodes in their bins; the outputs
// do not depend on their order. No floating-point atomics.
//
// radius_cells_fill stands for radius_fill (no nearest mode): the same slots
// written and the same left alone. One launch.
//
// radius_cells_sort_max: the kept edges of one dst that are ordered in LDS; a
// dst with more takes a slower exact path (for tests to aim at).
// radius_cells_min_nodes: the largest-sample size from which the store's
// "auto" takes this path.
int radius_cells_sort_max();
int radius_cells_min_nodes();
size_t radius_cells_scratch_bytes(int64_t nidx, int64_t ncap);
void radius_cells_count(hipStream_t stream, const void* d_pos, int pos_t,
                        const int64_t* d_ptr, int64_t nidx, int64_t ncap, float r,
                        int64_t max_neighbors, bool loop, void* d_scratch,
                        int64_t* d_edge_ptr);
void radius_cells_fill(hipStream_t stream, const void* d_pos, int pos_t,
                       const int64_t* d_ptr, const int64_t* d_edge_ptr, int64_t nidx,
                       int64_t ncap, int64_t ecap, float r, bool loop, void* d_scratch,
                       int out_t, bool coo, void* d_edge_out, float* d_vec_out);

// Periodic radius-graph fetch (DeviceStore::gather_radius_graph_pbc): as
// above, with the translated images of every node. d_cell is the (nidx, 9)
// array of cell_t (DDS_F32 or DDS_F64) the fixed-stride gather has just
// written for the same indices d_idx, row s the cell of request s (lattice
// vector a_k at 3k..3k+2); nsamples is the variable's global sample count, so
// a bad index, whose cell row was not written, is never read. pbc has bit k
// set for a periodic axis k; max_shift is in 1..8.
//
// Rule (docs/API.md): per graph needed_k = floor(q * (1 + 2^-10)) + 1 with q
// = r * |a_i x a_j| / |det| in f32, INT32_MAX for a zero-volume or non-finite
// cell, 0 on a non-periodic axis; b_k = min(max_shift, needed_k); the images
// are the triples s with |s_k| <= b_k. dx = (x_i - x_j) + t_x with t = (s0*a0
// + s1*a1) + s2*a2, nothing added for s = 0; d2 and r2 as above. (src = i,
// dst = j, s) is an edge iff d2 <= r2 and (i != j or s != 0 or loop). A
// graph's edges are ordered by dst, then s (lexicographic, ascending), then
// src.
//
// radius_pbc_count: d_edge_ptr as radius_count leaves it, and d_needed[3s..]
// = needed of request s, unclamped, 0 for a bad index and for a graph whose
// nodes were not kept. d_scratch: radius_pbc_scratch_bytes(nidx) bytes, no
// zeroing needed. Two launches.
//
// radius_pbc_fill: as radius_fill, and row d_edge_ptr[s] + e of the (ecap, 3)
// int32 array d_shift_out is the edge's s. One launch; no atomics and no
// counters in either.
//
// Nearest mode: as above with the key (d2 bits, image number * nodes + src),
// the image number counting the box in shift order; every graph needs nodes *
// images < 2^32, which the caller checks. radius_pbc_nearest_select stands
// for radius_pbc_count, radius_pbc_fill takes nearest = true, and both need
// radius_pbc_scratch_bytes(nidx, ncap, true) bytes.
size_t radius_pbc_scratch_bytes(int64_t nidx, int64_t ncap = 0, bool nearest = false);
void radius_pbc_nearest_select(hipStream_t stream, const void* d_pos, int pos_t,
                               const void* d_cell, int cell_t, const int64_t* d_ptr,
                               const int64_t* d_idx, int64_t nidx, int64_t nsamples,
                               int64_t ncap, float r, int pbc, int max_shift, bool loop,
                               int k, void* d_scratch, int64_t* d_edge_ptr,
                               int32_t* d_needed);
void radius_pbc_count(hipStream_t stream, const void* d_pos, int pos_t,
                      const void* d_cell, int cell_t, const int64_t* d_ptr,
                      const int64_t* d_idx, int64_t nidx, int64_t nsamples,
                      int64_t ncap, float r, int pbc, int max_shift, bool loop,
                      void* d_scratch, int64_t* d_edge_ptr, int32_t* d_needed);
void radius_pbc_fill(hipStream_t stream, const void* d_pos, int pos_t,
                     const int64_t* d_ptr, const int64_t* d_edge_ptr, int64_t nidx,
                     int64_t ncap, int64_t ecap, float r, int pbc, bool loop,
                     const void* d_scratch, int out_t, bool coo, void* d_edge_out,
                     int32_t* d_shift_out, float* d_vec_out, bool nearest = false);

// Cell-list path of the periodic fetch (docs/API.md, algorithm = "cells"): the
// same rule, order and outputs bit for bit, through the grid of the open
// cell-list path with a bin width per graph; real nodes only are binned, and
// every dst probes the images of its box. radius_pbc_cells_count stands for
// radius_pbc_count (d_edge_ptr and d_needed as it leaves them),
// radius_pbc_cells_fill for radius_pbc_fill without the nearest mode.
// d_scratch: radius_pbc_cells_scratch_bytes(nidx, ncap) bytes, under 112 *
// ncap + 168 * nidx + 288 whatever the cells and coordinates are, 16-byte
// aligned, no zeroing needed. Needs ncap + nidx < 2^31 and nodes * images <
// 2^32 per graph, which the caller checks. Integer atomics place the nodes in
// their bins; no floating-point atomics.
size_t radius_pbc_cells_scratch_bytes(int64_t nidx, int64_t ncap);
void radius_pbc_cells_count(hipStream_t stream, const void* d_pos, int pos_t,
                            const void* d_cell, int cell_t, const int64_t* d_ptr,
                            const int64_t* d_idx, int64_t nidx, int64_t nsamples,
                            int64_t ncap, float r, int pbc, int max_shift, bool loop,
                            void* d_scratch, int64_t* d_edge_ptr, int32_t* d_needed);
void radius_pbc_cells_fill(hipStream_t stream, const void* d_pos, int pos_t,
                           const int64_t* d_ptr, const int64_t* d_edge_ptr, int64_t nidx,
                           int64_t ncap, int64_t ecap, float r, bool loop, void* d_scratch,
                           int out_t, bool coo, void* d_edge_out, int32_t* d_shift_out,
                           float* d_vec_out);

// Triplet index of a radius-graph batch (DeviceStore::build_triplets). The
// input is what radius_fill / radius_pbc_fill and graph_fill have written on
// the same stream: d_edge_index the (2, ecap) ids of id_t (DDS_I64 or DDS_I32;
// anything else launches nothing), d_shift the (ecap, 3) int32 image shifts or
// nullptr (all zero), d_ptr / d_edge_ptr the [nidx+1] offsets. It is trusted
// as their output -- a graph's edges ordered by dst, then shift, then src,
// ids shifted by d_ptr[s] -- and not validated; ids out of range and unordered
// runs give wrong triplets, never an access outside the arrays.
//
// Rule (docs/API.md, "Triplets"): graph s is kept iff d_ptr[s+1] <= ncap and
// d_edge_ptr[s+1] <= ecap. A kept edge e = (j -> i, shift s_e) forms the
// triplet (e', e) with every column e' of its graph whose dst is j, except the
// one with src == i and shift == -s_e; triplets are ordered by e, then e'.
//
// triplet_count: d_trip_ptr[0..nidx] = exclusive scan of the per-graph triplet
// counts, 0 for a graph that is not kept, never clamped by any capacity; the
// per-edge offsets, run starts and excluded columns stay in d_scratch. Four
// launches (three without edges). d_scratch: triplet_scratch_bytes(nidx, ncap,
// ecap) bytes, no zeroing needed, independent of the number of triplets.
//
// triplet_fill: every element of the (2, tcap) output d_out of id_t. Row 0 is
// e', row 1 is e, for the triplets of every kept graph with d_trip_ptr[s+1] <=
// tcap, at columns d_trip_ptr[s] onwards; every other slot = trip_fill. 16-B
// stores when tcap % 4 == 0 and d_out is 16-B aligned, element stores
// otherwise. d_scratch and the other arguments are triplet_count's, on the
// same stream. One launch; no atomics, no counters, no waiting between
// workgroups in either.
//
// triplet_slice: the edges whose offsets one tile of the fill stages in LDS; a
// tile that spans more (edges without triplets) searches them in global memory
// (a second code path, for tests to aim at).
int triplet_slice();
size_t triplet_scratch_bytes(int64_t nidx, int64_t ncap, int64_t ecap);
void triplet_count(hipStream_t stream, const void* d_edge_index, int id_t,
                   const int32_t* d_shift, const int64_t* d_ptr,
                   const int64_t* d_edge_ptr, int64_t nidx, int64_t ncap, int64_t ecap,
                   void* d_scratch, int64_t* d_trip_ptr);
void triplet_fill(hipStream_t stream, const int64_t* d_ptr, const int64_t* d_edge_ptr,
                  const int64_t* d_trip_ptr, int64_t nidx, int64_t ncap, int64_t ecap,
                  int64_t tcap, const void* d_scratch, int id_t, int64_t trip_fill,
                  void* d_out);

// MX (OCP microscaling v1.0) block-scaled storage. A variable of logical
// width `disp` keeps each row packed as
//   [nblk * 32 element codes][nblk E8M0 scale bytes][zero pad to 16 B]
// with nblk = ceil(disp / 32); fp8 codes take a byte, e2m1 codes a nibble
// (even column low). The packed row is an ordinary DDS_U8 row of
// mx_row_bytes() bytes, so everything that moves rows moves it unchanged.
enum DDSMxElem : int { DDS_MX_E4M3 = 0, DDS_MX_E5M2 = 1, DDS_MX_E2M1 = 2 };
inline int64_t mx_payload_bytes(int64_t disp, int elem) {
    return (disp + 31) / 32 * (elem == DDS_MX_E2M1 ? 16 : 32);
}
inline int64_t mx_row_bytes(int64_t disp, int elem) {
    return (mx_payload_bytes(disp, elem) + (disp + 31) / 32 + 15) / 16 * 16;
}

// gather_rows for an MX variable: rows of mx_row_bytes(disp, elem) bytes are
// gathered, dequantized (code * 2^(scale byte - 127), scale byte 255 = NaN),
// run through `xf` (affine columns are logical columns, d_scale / d_shift
// hold `disp` floats) and cast to out_t, which must be DDS_F32, DDS_F16 or
// DDS_BF16 (anything else launches nothing). d_out holds nidx * disp
// elements; out-of-range indices are skipped and counted in d_oob.
void gather_rows_mx(hipStream_t stream, const RowDir& dir, const int64_t* d_idx,
                    int64_t nidx, int64_t disp, int elem, int out_t, const Affine& xf,
                    void* d_out, unsigned long long* d_oob);

// The fetches of an MX CSR variable: a CSR variable of DDS_U8 whose elements
// are packed rows of mx_row_bytes(disp, elem) bytes (`dir` describes that
// variable). Elements are dequantized, run through `xf` (affine columns are
// logical columns in [0, disp)) and cast to out_t, which must be DDS_F32,
// DDS_F16 or DDS_BF16 (anything else launches nothing), in one launch each, no
// scratch. `mean_len` is the variable's mean sample length in elements; it
// only sizes the lane group.
//
// gather_csr_mx, the packed placement: sample d_idx[s] goes to rows
// d_out_off[s] .. d_out_off[s+1] of a (cap_elems, disp) output. d_out_off
// must come from csr_offsets on the same stream, which has counted the bad
// indices and ADDED the requested total to d_ctrs[DDS_CTR_ELEMS]; this is
// gather_csr_balanced's capacity rule: a sample with L > 0 elements whose
// slice would end past cap_elems is not written, counts once in
// d_ctrs[DDS_CTR_CAP], and takes its L elements back out of DDS_CTR_ELEMS.
// d_out_off is read, never clamped. So DDS_CTR_ELEMS * mx_row_bytes is the
// packed bytes read.
void gather_csr_mx(hipStream_t stream, const CsrDir& dir, const int64_t* d_idx,
                   int64_t nidx, const int64_t* d_out_off, int64_t disp, int elem,
                   int64_t mean_len, int out_t, const Affine& xf, int64_t cap_elems,
                   void* d_out, unsigned long long* d_ctrs);

// gather_csr_padded_mx, the padded placement, gather_csr_padded's contract:
// sample d_idx[s] is written to row s of a dense (nidx, max_len, disp) output,
// its first min(len, max_len) elements decoded, the rest of the row filled
// with the raw `pad_bits` of one output element; d_lengths[s] gets the true
// length. An out-of-range index gives an all-pad row, length 0 and one count
// in d_ctrs[DDS_CTR_OOB]; sum(min(len, max_len)) accumulates into
// d_ctrs[DDS_CTR_ELEMS]. Every output element is written exactly once.
void gather_csr_padded_mx(hipStream_t stream, const CsrDir& dir, const int64_t* d_idx,
                          int64_t nidx, int64_t disp, int elem, int64_t mean_len,
                          int64_t max_len, int out_t, const Affine& xf, uint64_t pad_bits,
                          void* d_out, int64_t* d_lengths, unsigned long long* d_ctrs);

// Quantize `nrows` rows of `disp` values (in_t DDS_F32, DDS_F16 or DDS_BF16,
// device memory, contiguous) into packed MX rows at d_dst, by the rule in
// docs/API.md ("MX storage"). Every byte of every packed row is written, and
// the bytes are a pure function of the input.
void quantize_rows_mx(hipStream_t stream, const void* d_src, int in_t, int64_t nrows,
                      int64_t disp, int elem, void* d_dst);

// Dense narrowing cast of `n_elems` contiguous elements, d_dst[i] =
// cast(d_src[i]) by the rule the casting gathers use (docs/API.md, cast
// semantics; f64 -> f16/bf16 rounds through f32). Supported pairs
// (cast_rows_supported): DDS_F64 -> DDS_F32 / DDS_F16 / DDS_BF16 and DDS_F32
// -> DDS_F16 / DDS_BF16; any other pair launches nothing. Both pointers are
// device memory aligned to their element; one launch on `stream`.
bool cast_rows_supported(int in_t, int out_t);
void cast_rows(hipStream_t stream, const void* d_src, void* d_dst, int64_t n_elems,
               int in_t, int out_t);

// Scatter rows of a packed buffer into the local shard at arbitrary local row
// ids (inverse of gather_rows with nparts==1). Used by the epoch reshuffle to
// place all-to-all-received rows.
void scatter_rows_local(hipStream_t stream,
                        void* d_base, int64_t nrows_local,
                        int64_t row_elems, int elem_t,
                        const int64_t* d_local_idx, int64_t nidx,
                        const void* d_src, unsigned long long* d_oob);

} // namespace ddstore
