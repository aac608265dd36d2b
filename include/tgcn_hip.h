/* tgcn_hip.h -- C ABI of libtgcn_hip.so: the Chebyshev (time-)graph convolution hot path of
 * cassianobecker/tgcn as hand-written HIP for gfx950 (MI355X).
 *
 * The reference has no native layer: its "operator API" for this path is the Python class surface of
 * tgcn/nn/gcn.py (TGCNCheb :8, TGCNCheb_H :82, GCNCheb :158, ChebConv :348, ChebTimeConv :445) and
 * gcn/graph.py::chebyshev (:241).  The entry points below are what a maintainer of the reference would
 * bind (ctypes) to replace the stock-torch ops inside those forwards; every entry
 * point names the reference lines it replaces.
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer owned by the caller; fp32, row-major, last dim contiguous
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); NULL = default
 *   - nothing allocates, frees or synchronises; scratch comes from the caller (see *_workspace_bytes)
 *   - returns 0 on success, a negative TGCN_ERR_* code otherwise; tgcn_last_error() gives the text
 *     (thread-local).  Nothing throws across the ABI.  Launches go to the calling thread's current device.
 */
#ifndef TGCN_HIP_H
#define TGCN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TGCN_OK 0
#define TGCN_ERR_INVALID (-1)     /* bad argument (shape, alignment, null pointer) */
#define TGCN_ERR_LAUNCH (-2)      /* HIP launch error */
#define TGCN_ERR_WORKSPACE (-3)   /* caller workspace too small */
#define TGCN_ERR_UNSUPPORTED (-4) /* shape outside what the kernels were built for */

#define TGCN_ABI_VERSION 8

/* One stored entry of the sparse operand: 8 bytes, read with a single load. */
typedef struct tgcn_edge {
  int32_t col;
  float val;
} tgcn_edge;

/* CSR operand L-hat (n x n).  Replaces the dense (n,n) `self.L` of gcn.py:18,92,168 and the per-call
 * (edge_index, lap) pair of gcn.py:413,510. */
typedef struct tgcn_csr {
  int64_t n;
  int64_t nnz;           /* < 2^31 */
  const int32_t* rowptr; /* [n+1] */
  const tgcn_edge* edges; /* [nnz], rows in order */
  const float* dense;    /* optional (null if absent): the same operand as a row-major n x n fp32 matrix, duplicates
                            summed.  Only read for small dense operands (n <= 256 with >= n*n/4 stored entries), which
                            then run on the matrix pipe (tgcn_cheb_forward_small_f32 / tgcn_cheb_basis_small_f32). */
} tgcn_csr;

/* Work schedule of one operand for one lane-group width (built once by the host side, tgcn_amd/graph.py).
 *   rows with <= row_thresh stored entries: nnz-balanced row blocks, one workgroup each, one lane group per row;
 *   longer rows: segments of bounded length, STORED IN ORDER OF THEIR FIRST COLUMN so that the groups in flight
 *   gather from the same region of the dense operand at about the same time (hub columns then hit in L2).
 *   16-lane schedules: rows of more than row_thresh but at most 128 entries are one whole-row segment handled by ONE WAVE (nwseg);
 *   where the partial rows of the longer rows would not fit the Infinity Cache (npartial * lanes_per_row * 16 B > 256 MiB), rows of more
 *   than 512 entries ("hub rows") are cut into wave segments of 64 consecutive entries, one WAVE and one scratch slot each (nwseg too).
 *   A segment that is its whole row writes the row directly (seg_slot = -1); rows cut into several segments
 *   ("long rows") sum them through numbered scratch slots that a fix-up launch folds in slot order, so results
 *   do not depend on timing.  The first nhuge long rows (most slots) get a whole workgroup each in the fix-up.
 *   seg_mode 0: one lane group per segment (segments of <= 32 entries).  seg_mode 1 (lanes_per_row < 64): one WAVE per
 *   segment of <= 32 * (64 / lanes_per_row) entries -- its lane groups take consecutive pieces and the pieces are folded
 *   inside the wave, so rows up to that length are written directly and longer rows leave one partial row per wave. */
typedef struct tgcn_csr_sched {
  int32_t lanes_per_row; /* lane-group width the schedule was balanced for: 1,2,4,...,64 */
  int32_t row_thresh;
  int32_t nblk;     /* row blocks */
  int32_t nseg;     /* segments */
  int32_t nlong;    /* rows cut into more than one segment */
  int32_t nhuge;    /* leading entries of long_row folded by a whole workgroup */
  int32_t npartial; /* scratch slots (= segments of long rows) */
  int32_t seg_mode; /* 0 lane-group segments, 1 wave segments */
  int32_t row_mix;  /* 1: row blocks dealt evenly among the segment blocks instead of all in front -- set by the builders for operands with
                       >= 1/8 structurally empty rows, whose row blocks are mostly streaming zero writes that fill the gaps of the
                       gather-bound segments (uncompacted R-MAT: 4.25 -> 3.95 ms per launch); 0 otherwise (it costs 2.5 % there) */
  int32_t nwseg;    /* leading entries of the seg_* arrays that are handled by ONE WAVE each (its lane groups take consecutive quarters of the
                       segment, folded inside the wave; the builders use them for 16-lane schedules only).  Two runs, each in order of first
                       column: first the WHOLE rows of row_thresh < entries <= 32 * (64 / lanes_per_row), seg_slot = -1, written directly -- no
                       partial rows, no fix-up for them; behind them the hub rows' wave segments, seg_slot >= 0, one partial row per wave.  The
                       kernel asks nothing of the order or the lengths: any segment among the first nwseg is folded inside its wave and goes
                       where its seg_slot says.  The remaining nseg - nwseg entries are the lane-group segments of the other long rows.
                       0 for 64-lane schedules */
  const int32_t* blk_row;   /* [nblk+1] first row of each block; blk_row[nblk] == n */
  const int32_t* seg_row;   /* [nseg] */
  const int32_t* seg_e0;    /* [nseg] first entry */
  const int32_t* seg_e1;    /* [nseg] one past last entry */
  const int32_t* seg_slot;  /* [nseg] scratch slot (slots of one row are consecutive, in entry order, whichever kind of segment holds them), or -1: whole row, written directly */
  const int32_t* long_row;  /* [nlong] */
  const int32_t* long_slot; /* [nlong+1] first slot of each long row (slots of a row are consecutive, in column order) */
} tgcn_csr_sched;

/* Batched dense operand: element (b, i, c) lives at ptr[b*batch_stride + i*row_stride + c]. */
typedef struct tgcn_dense {
  float* ptr;
  int64_t batch_stride;
  int64_t row_stride;
} tgcn_dense;

const char* tgcn_last_error(void);
int tgcn_abi_version(void);

/* Operand and schedule construction inside the library (tgcn_graph_create_from_coo/csr, tgcn_graph_destroy),
 * so that a caller of the C ABI needs nothing from the Python package.  The work runs ON THE DEVICE in kernels of this library
 * (csrc/device_build.h: stable LSD radix sort, prefix sums, binary-search marks -- no host round trip of the index arrays);
 * these are the ONLY entry points that allocate device memory and synchronise (a few 8-byte read-backs that size the next
 * allocation): call them once per graph, outside the forward path.  All index / value pointers are DEVICE pointers.
 *   from_coo         entries in any order; duplicates of one (row, col) stay separate entries in their given order (their
 *                    sum is what scatter_add computes, gcn.py:308,343)
 *   from_csr         the same from row pointers (int64, rowptr[n] = nnz)
 *   from_edge_index  the operand ChebConv / ChebTimeConv build on every forward (gcn.py:398-413 == :495-510) from the
 *                    caller's (2, E) int64 edge list and optional weights: self loops removed, source-degree normalised
 *   tgcn_sched_build the row-block + column-ordered-segment schedule of tgcn_csr_sched for rows of C floats (what
 *                    tgcn_amd/graph.py::Schedule builds) */
typedef struct tgcn_graph tgcn_graph; /* opaque: owns its device arrays */
typedef struct tgcn_sched tgcn_sched; /* opaque: owns its device arrays */
int tgcn_graph_create_from_coo(int64_t n, int64_t n_cols, int64_t nnz, const int64_t* row, const int64_t* col, const float* val,
                               tgcn_graph** out);
int tgcn_graph_create_from_csr(int64_t n, int64_t n_cols, const int64_t* rowptr, const int32_t* col, const float* val,
                               tgcn_graph** out);
int tgcn_graph_create_from_edge_index(int64_t n, int64_t E, const int64_t* edge_index, const float* edge_weight,
                                      tgcn_graph** out);
const tgcn_csr* tgcn_graph_csr(const tgcn_graph* g);
int64_t tgcn_graph_n_cols(const tgcn_graph* g);
void tgcn_graph_destroy(tgcn_graph* g);
int tgcn_sched_build(const tgcn_graph* g, int32_t C, int aligned16, tgcn_sched** out);
/* The same schedule for a CSR the caller owns (n_cols = number of columns of the operand). */
int tgcn_sched_build_csr(const tgcn_csr* A, int64_t n_cols, int32_t C, int aligned16, tgcn_sched** out);
/* The arrays of a library-built schedule copied (device to device) into arrays the caller owns, sized from the counts of
 * tgcn_sched_get: blk_row [nblk+1], seg_row / seg_e0 / seg_e1 / seg_slot [max(nseg, 1)], long_row [max(nlong, 1)],
 * long_slot [max(nlong + 1, 2)].  Lets a host side that manages its own memory (tgcn_amd/graph.py) drop the handle afterwards. */
int tgcn_sched_copy(const tgcn_sched* s, void* stream, int32_t* blk_row, int32_t* seg_row, int32_t* seg_e0, int32_t* seg_e1,
                    int32_t* seg_slot, int32_t* long_row, int32_t* long_slot);
/* COO -> CSR into CALLER memory on `stream` (what tgcn_graph_create_from_coo does into memory of its own): rowptr [n+1] int32 and
 * packed entries [nnz], rows sorted by (row, col), duplicates in their given order.  Device kernels of this library (two stable
 * radix sorts, a prefix sum); synchronises the stream once (range check of the indices).  workspace: 256-byte aligned,
 * tgcn_csr_build_workspace_bytes(n, nnz). */
size_t tgcn_csr_build_workspace_bytes(int64_t n, int64_t nnz);
int tgcn_csr_build_f32(void* stream, int64_t n, int64_t n_cols, int64_t nnz, const int64_t* row, const int64_t* col, const float* val,
                       int32_t* rowptr, tgcn_edge* edges, void* workspace, size_t workspace_bytes);

/* ABI v5 -- the operand VALUES the callers compute before their layers, on caller memory (device pointers, `stream`), so that a host side
 * that owns its arrays (tgcn_amd/graph.py) has no arithmetic of its own: one builder, the library's.  Both synchronise the stream once
 * (range flag / count) and write a HOST count; workspace 256-byte aligned.
 *   tgcn_edge_normalise_f32       edge list (2, E) int64 [+ weights, nullable] -> COO of the ChebConv / ChebTimeConv operand
 *                                 (tgcn/nn/gcn.py:398-413 == :495-510): self loops removed, lap_e = -deg^-1/2[row] * w_e * deg^-1/2[col] with
 *                                 deg = UNWEIGHTED edge count per source vertex (integer atomics: order-independent), deg^-1/2 = 0 at degree 0.
 *                                 row / col / val: E slots; *kept entries are written, in the given order.  (tgcn_graph_create_from_edge_index
 *                                 is this followed by tgcn_graph_create_from_coo.)
 *   tgcn_adjacency_normalise_f32  COO of the weight matrix W (m entries, any order) -> COO of rescale_L(laplacian(W, normalized=True), lmax)
 *                                 (gcn/graph.py:117-136, 232-238): d = colsum(W) + eps -- a stable sort by column, then one wave per column in a
 *                                 fixed summation order, no float atomics --, L-hat = (2/lmax) (I - D^-1/2 W D^-1/2) - I.  row_out / col_out /
 *                                 val_out: m + n slots; *count = m, plus n diagonal entries when lmax != 2. */
size_t tgcn_edge_normalise_workspace_bytes(int64_t n, int64_t E);
int tgcn_edge_normalise_f32(void* stream, int64_t n, int64_t E, const int64_t* edge_index, const float* edge_weight, int64_t* row, int64_t* col,
                            float* val, int64_t* kept, void* workspace, size_t workspace_bytes);
size_t tgcn_adjacency_normalise_workspace_bytes(int64_t n, int64_t m);
int tgcn_adjacency_normalise_f32(void* stream, int64_t n, int64_t m, const int64_t* row, const int64_t* col, const float* weight, float lmax,
                                 int64_t* row_out, int64_t* col_out, float* val_out, int64_t* count, void* workspace, size_t workspace_bytes);

/* One level of the reference's Graclus / METIS-style coarsening (gcn/coarsening.py:119-165: a Python loop over vertices and
 * entries) as host code: HOST arrays in and out -- coarsening is one-off preprocessing of the caller's graph (tgcn_amd/
 * coarsening.py mirrors coarsen / metis / compute_perm / perm_data / perm_adjacency around it).  Entries sorted by row;
 * `order` = visiting sequence; an unmatched vertex v joins the unmatched neighbour u with the largest
 * vv * (1/weight[v] + 1/weight[u]) (first one in entry order on ties), in float / double arithmetic like the reference's
 * dtype; cluster[v] = cluster index in visiting order. */
int tgcn_graclus_match_f32(int64_t nnz, const int64_t* rr, const int64_t* cc, const float* vv, int64_t n, const int64_t* order,
                           const float* weight, int32_t* cluster);
int tgcn_graclus_match_f64(int64_t nnz, const int64_t* rr, const int64_t* cc, const double* vv, int64_t n, const int64_t* order,
                           const double* weight, int32_t* cluster);
const tgcn_csr_sched* tgcn_sched_get(const tgcn_sched* s);
void tgcn_sched_destroy(tgcn_sched* s);

/* Optional launch timing for benchmarks: between start and stop every kernel launch THE CALLING THREAD makes through this
 * library is bracketed by a hipEvent pair on its own stream.  stop() (same thread) synchronises those events and returns
 * (kind, milliseconds) per launch in launch order.  Thread-local since ABI v7: launches of other threads (DataParallel replicas,
 * autograd workers running a backward) are not recorded and never touch the record.  Not for use under hipGraph capture. */
#define TGCN_PROF_HOP 0
#define TGCN_PROF_HOP_FIXUP 1
#define TGCN_PROF_PROJECT 2
#define TGCN_PROF_RELAYOUT 3
#define TGCN_PROF_SMALL 4
#define TGCN_PROF_WGRAD 5
#define TGCN_PROF_SMALL_BASIS 6
/* 7 and 8 are not used: they named the launches of the fused last hop, removed in ABI v8 */
int tgcn_profile_start(int32_t capacity);
int tgcn_profile_stop(int32_t* kinds, float* ms, int32_t capacity, int32_t* count);

/* Developer switches for A/B runs (tools/hop_bench.py, tools/proj_bench.py; every one is checked against the oracle in
 * tests/test_fuzz_parity.py).  State of the CALLING THREAD since ABI v7 (thread_local in the library, as is the launch-timing record of
 * tgcn_profile_*): a switch changes the launches the calling thread issues afterwards and nothing else -- the threads of an
 * nn.DataParallel process (examples/pytorch_based/pytorch_hcp_tgcn.py:270-273) and the autograd engine's workers keep the defaults,
 * which are what ships; the library holds no process-global mutable state, only caches of immutable per-device facts
 * (CU count, the LDS attribute of a kernel).  Same arithmetic, another kernel; TGCN_ERR_INVALID for unknown keys.
 *   "hop_variant"     0 shipped hop kernel; 1.. alternative unroll / row-interleave shapes of hop.h
 *   "hop_xcd_remap"   1 (default): each XCD gets a contiguous range of row blocks; 0: row blocks round robin over the XCDs
 *   "hop_seg_remap"   1: each XCD gets a contiguous range of the column-ordered segment blocks; 0 (default): round robin
 *   "hop_mix"         0 (default): row blocks in front unless the schedule asks for the mix (tgcn_csr_sched.row_mix); 1: always dealt among
 *                     the segment blocks; 2: segment blocks first
 *   "hop_stream"      1 (default): outputs larger than the Infinity Cache (256 MB) take the form with non-temporal entry loads, row
 *                     stores and partial-row stores (16-lane groups); 0: plain accesses always
 *   "hop_lds_pad"     bytes of unused dynamic LDS per hop_kernel workgroup: limits the workgroups per CU to 160 KB / pad (0: none)
 *   "project_variant" 0 auto; 1 exact-fp32 streaming-W; 2 exact-fp32 W-resident with 16-row wave tiles; 3 bf16x3 always;
 *                     4 exact-fp32 auto; 5 vector-ALU narrow kernel wherever it applies
 *   "x3_form"         2 (default) bf16x3 with A fragments from registers for >= 96 output columns; 1 both operands via LDS
 *   "x3_tail"         1 (default): the rows of a thinly filled last round of the wide bf16x3 kernel go out as 128-row tiles; 0: never
 *   "small_dense"     dense small operands: 2 (default) bf16x3 on the matrix pipe when the batch fills the chip, 1 exact
 *                     fp32 MFMA only, 0 vector-ALU one-launch kernels
 *   "small_narrow"    0: C <= 4 inputs use the output-side one-launch kernel (default 1: input-side recursion)
 *   "x3_stream_cap"   workgroups of the co-schedulable streaming projection (0, default: one per two CUs)
 *   "compact_overlap" 1 (default): the compacted fp32 layer runs projections on the library's side stream beside its hop launches
 *                     where that pays; 0: everything on the caller's stream, one kernel after the other
 *   "compact_overlap_group"   time steps per group (default 3): a group's projection runs beside the next group's hops
 *   "compact_overlap_min_mb"  ... only when one time step's compact hop tensor is larger than this (default 256, the Infinity Cache)
 *   "sched_hub_min"   tgcn_sched_build*, 16-lane schedules: rows of more entries are hub rows, cut into wave segments (default 512; 0: none) ...
 *   "sched_hub_seg"   ... of this many entries (default 64; at least 32 and at most sched_hub_min, else no hub rows) ...
 *   "sched_hub_gate_mb"  ... where the partial rows of the schedule without hub rows take more than this many MiB (default 256, the
 *                     Infinity Cache; 0: always).  Read when a schedule is built; tgcn_amd/graph.py: HUB_MIN, HUB_SEG, HUB_GATE_BYTES */
int tgcn_set_tuning(const char* key, int32_t value);
/* Every switch above back to its default, for the calling thread (ABI v5; thread-local since v7).  A harness that sets one restores
 * them with this call in its teardown, whatever happened in between (tests/conftest.py does after every test). */
void tgcn_reset_tuning(void);

/* Geometry the host needs to build a schedule / size scratch for a row length C (floats).
 * `aligned16` != 0 when every operand base, row stride and batch stride is a multiple of 4 floats. */
int tgcn_hop_vec_width(int32_t C, int aligned16);      /* floats per lane: 4 or 1 */
int tgcn_hop_lanes_per_row(int32_t C, int aligned16);  /* 1,2,...,64 */
int tgcn_hop_groups_per_block(int32_t C, int aligned16); /* 256 / lanes_per_row */
size_t tgcn_csr_hop_workspace_bytes(const tgcn_csr_sched* sched, int32_t nb, int32_t C, int aligned16);

/* One hop of the recursion:  S = L-hat . X ;  P = S (optional) ;  Y = alpha*S + beta*Z (Z optional).
 *   reference_power (gcn.py:72-78,147-153,230-236):  P_k = L P_{k-1};  Xt[k] = 2 P_k - Xt[k-2]
 *   chebyshev       (gcn.py:423-431,521-527):        Tx_k = 2 L Tx_{k-1} - Tx_{k-2}
 *   plain SpMM      (gcn.py:258-345 spmm*):          alpha=1, Z=NULL
 * nb batches of (n x C) rows share the CSR. */
int tgcn_csr_hop_f32(void* stream, const tgcn_csr* A, const tgcn_csr_sched* sched, int32_t nb, int32_t C,
                     const tgcn_dense* X, const tgcn_dense* Z, float alpha, float beta, const tgcn_dense* Y,
                     const tgcn_dense* P, void* workspace, size_t workspace_bytes);

/* tgcn_csr_hop_f32 with a second addend:  Y = alpha*S + beta*Z + gamma*Z2  (Clenshaw step of the project-first path). */
int tgcn_csr_hop2_f32(void* stream, const tgcn_csr* A, const tgcn_csr_sched* sched, int32_t nb, int32_t C,
                      const tgcn_dense* X, const tgcn_dense* Z, float alpha, float beta, const tgcn_dense* Z2, float gamma,
                      const tgcn_dense* Y, const tgcn_dense* P, void* workspace, size_t workspace_bytes);

/* ---- bf16 operands (the layers' bf16 path: a bf16 weight picks it; DESIGN.md "bf16 layers").  Element codes of the dtype flags: */
#define TGCN_DTYPE_F32 0
#define TGCN_DTYPE_BF16 1

/* tgcn_csr_hop_f32 / tgcn_csr_hop2_f32 on rows of bf16 elements: X, Z, Z2, Y, P hold bf16 (tgcn_dense.ptr points at them, strides in
 * ELEMENTS); the CSR values stay fp32.  Each row is accumulated in fp32 and rounded once, to nearest even, when it is stored; the partial
 * rows of long rows in the workspace are fp32.  Geometry is keyed on row bytes: with every base 16-byte aligned and strides multiples of
 * 8 elements (aligned16 != 0) and C % 8 == 0, a lane moves 8 elements and `sched` must be the schedule an fp32 row of C/2 floats takes
 * (tgcn_hop_lanes_per_row(C/2, 1)); otherwise one element per lane, the schedule of tgcn_hop_lanes_per_row(C, 0). */
size_t tgcn_csr_hop_bf16_workspace_bytes(const tgcn_csr_sched* sched, int32_t nb, int32_t C, int aligned16);
int tgcn_csr_hop_bf16(void* stream, const tgcn_csr* A, const tgcn_csr_sched* sched, int32_t nb, int32_t C,
                      const tgcn_dense* X, const tgcn_dense* Z, float alpha, float beta, const tgcn_dense* Y,
                      const tgcn_dense* P, void* workspace, size_t workspace_bytes);
int tgcn_csr_hop2_bf16(void* stream, const tgcn_csr* A, const tgcn_csr_sched* sched, int32_t nb, int32_t C,
                       const tgcn_dense* X, const tgcn_dense* Z, float alpha, float beta, const tgcn_dense* Z2, float gamma,
                       const tgcn_dense* Y, const tgcn_dense* P, void* workspace, size_t workspace_bytes);

/* The same hop in fp64 for the numpy twin gcn.graph.chebyshev(L, X, K) with a float64 operand: the reference computes in
 * L.dtype (gcn/graph.py:247, 256-265).  Plain CSR (int32 rowptr / col, fp64 val), X / Z / Y / P: rows of F contiguous doubles;
 * Y = alpha * (L X) + beta * Z (Z nullable), P = L X (nullable).  Entries are summed in stored order. */
int tgcn_csr_hop_f64(void* stream, int64_t n, const int32_t* rowptr, const int32_t* col, const double* val, int64_t F,
                     const double* X, const double* Z, double alpha, double beta, double* Y, double* P);

/* Change of basis of a (K, CN) weight between the dense-L classes' recursion Xt[k] = 2 L^k x - Xt[k-2] (gcn.py:75-78) and the
 * monomials L^j x the kernels work in:  out[j, :] = sum_k fold[k, j] W[k, :]  (transpose != 0: sum_k fold[j, k] W[k, :], the
 * adjoint, for the weight gradient).  fold: K x K device matrix (tgcn_amd/functional.py::power_fold_matrix). */
int tgcn_fold_weight_f32(void* stream, int32_t K, int64_t CN, const float* fold, const float* W, float* out, int32_t transpose);

/* Re-layouts of a (K, C, N) layer weight for the drivers (ABI v6; the host side issues no torch permute on the path):
 *   kind 0: (C, K*N), out[c, k*N + n] = W[k, c, n]  -- Wcat of tgcn_cheb_forward_pf_f32;
 *   kind 1: (K, N, C), W_k^T -- the input gradient as a layer on (L^T, g, W^T);   kind 2: (N, K*C) -- G = g [W_0^T | ... | W_{K-1}^T]. */
int tgcn_weight_layout_f32(void* stream, int32_t K, int32_t C, int32_t N, const float* W, float* out, int32_t kind);

/* Stacked-hop dense projection (gcn.py:39,113,194 einsum; :420-431 / :519-527 per-hop matmul):
 *   out[r(m), :] (+)= sum_t A_t[m, 0:Kc] . W[t*Kc:(t+1)*Kc, 0:N] + bias
 * A_t: M x Kc with row stride lda[t]; W: (nterms*Kc) x N contiguous; fp32 MFMA, fp32 accumulate.
 * Row map r(m) = (m % interleave) * n_vertices + m / interleave   (interleave = 1: identity).
 * bias_kind: 0 none | 1 per channel [N] | 2 per vertex and channel [n_vertices*N] (vertex = r % n_vertices).
 * `a` and `lda` are HOST arrays of length nterms (<= 32). */
int tgcn_cheb_project_f32(void* stream, int64_t M, int32_t Kc, int32_t N, int32_t nterms, const float* const* a,
                          const int64_t* lda, const float* W, const float* bias, int32_t bias_kind,
                          int64_t n_vertices, int64_t interleave, int32_t accumulate, float* out, int64_t ldo);

/* The same contraction through a ROW MAP (ABI v5; the building block of the compacted layers): tile row m is the caller's
 * vertex rowmap[m] -- its output row, its bias row, and its row in every term t whose bit t is set in `mapped_terms` (typically term 0 = x in
 * the caller's labels); the other terms (compact hop tensors) are read at row m.  nbatch samples share the tile rows: sample b reads term t
 * at a[t] + b * a_bs[t] floats and writes out + b * out_bs (a per-vertex bias row then reaches HBM once per pass).  a_bs: HOST array of
 * nterms strides (nullable for nbatch = 1).  M = number of mapped rows (one sample); n_vertices = rows of the bias / output per sample.
 * interleave > 1 (vertex-major operands of the layout-1 driver, nbatch = 1): tile row m = (mapped vertex m / interleave, sample m % interleave),
 * M = mapped vertices x interleave; a mapped term is read at row rowmap[v] * interleave + s, the output row is s * n_vertices + rowmap[v].
 * This form exists in the vector-ALU kernel only (nterms * Kc <= 16 scalars per row, N % 4 == 0, M >= 4096): TGCN_ERR_UNSUPPORTED otherwise. */
int tgcn_cheb_project_mapped_f32(void* stream, int64_t M, int32_t Kc, int32_t N, int32_t nterms, const float* const* a, const int64_t* lda,
                                 const float* W, const float* bias, int32_t bias_kind, int64_t n_vertices, int64_t interleave, const int32_t* rowmap,
                                 uint32_t mapped_terms, int32_t nbatch, const int64_t* a_bs, int64_t out_bs, float* out, int64_t ldo);

/* tgcn_cheb_project_mapped_f32 at interleave = 1 through the STREAMING bf16x3 kernel, whatever the number of rows (rows of 32 / 64 floats,
 * N <= 64, 16-byte aligned operands and strides, no more weight than the LDS holds: TGCN_ERR_UNSUPPORTED otherwise); rowmap nullable.
 * tile_counter == NULL: the form the dispatch takes on its own (1024-thread workgroups, one per CU, tiles dealt round robin).
 * tile_counter != NULL (4 bytes of device memory, zeroed by this call on `stream`): the co-schedulable form the compacted layer runs beside
 * its hop launches -- 256-thread workgroups, by default one per two CUs ("x3_stream_cap"), whose waves claim their tiles from the counter.  Both forms
 * give the same bits. */
int tgcn_cheb_project_stream_f32(void* stream, int64_t M, int32_t Kc, int32_t N, int32_t nterms, const float* const* a, const int64_t* lda,
                                 const float* W, const float* bias, int32_t bias_kind, int64_t n_vertices, const int32_t* rowmap, uint32_t mapped_terms,
                                 int32_t nbatch, const int64_t* a_bs, int64_t out_bs, float* out, int64_t ldo, int32_t* tile_counter);

/* Kernels the calling thread has launched on the library's side stream so far (the compacted layer's projections beside the hops; none
 * while the caller's stream is being captured, on small operands, or with "compact_overlap" = 0). */
int64_t tgcn_side_stream_launches(void);

/* Streaming time windows (replaces materialising the T-H+1 overlapping windows of
 * load/data_hcp.py:116-154 and running TGCNCheb_H on each): series[t] are the hop tensors of ONE recording,
 * (n_vertices, T) contiguous (term t = L^t applied to the raw series); window w of vertex i is series[t][i, w:w+H].
 *   out[w, i, :] = sum_t series[t][i, w:w+H] . W[t*H:(t+1)*H, :] + bias       out: (T-H+1, n_vertices, N)
 * i.e. exactly what the layer returns for the windowed batch, with the K-1 hops done once on T columns instead
 * of (T-H+1)*H. */
int tgcn_cheb_project_windows_f32(void* stream, int64_t n_vertices, int32_t T, int32_t H, int32_t N, int32_t nterms,
                                  const float* const* series, const float* W, const float* bias, int32_t bias_kind,
                                  float* out);

/* Backward of tgcn_cheb_project_windows_f32 for S recordings at once: stack (K, S, n_vertices, T) hop tensors, g the gradient
 * of the (S*(T-H+1), n_vertices, N) output, W (K*H, N).
 *   G  (nullable, (K, S, n_vertices, T)):  G[k, s, i, t] = sum_h sum_c g[(s, t-h), i, c] W[k*H + h, c]  -- per-term input
 *      gradients, which the caller folds with the hop on L^T (Horner / Clenshaw, as for the layer)
 *   dW (nullable, (K*H, N)):  dW[k*H + h, c] = sum_{s,w,i} stack[k, s, i, w+h] g[(s, w), i, c]; fixed reduction order. */
size_t tgcn_cheb_windows_wgrad_workspace_bytes(int64_t S, int64_t n_vertices, int32_t T, int32_t H, int32_t N, int32_t K);
int tgcn_cheb_windows_backward_f32(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t H, int32_t N, int32_t K,
                                   const float* stack, const float* g, const float* W, float* G, float* dW, void* workspace,
                                   size_t workspace_bytes);

/* Streaming time windows of MULTI-CHANNEL series: stack (K, S, n_vertices, T*f) are the hop tensors of S recordings whose
 * time rows hold f contiguous channels; window w of vertex i is the H*f floats from float offset w*f of its row.  W: (K, H*f, N).
 *   out[(s, w, i), :] = sum_k stack[k, s, i, w*f : (w+H)*f] . W[k] + bias       one launch for all S recordings
 * as_series = 0: out is (S*(T-H+1), n_vertices, N), the order of tgcn_cheb_project_windows_f32; 1: (S, n_vertices, T-H+1, N), a series of
 * N channels that the next time layer streams over.  fp32 MFMA; bias_kind as in tgcn_cheb_project_f32 (2: [n_vertices*N]). */
int tgcn_cheb_project_series_f32(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                 const float* stack, const float* W, const float* bias, int32_t bias_kind, int32_t as_series, float* out);

/* Backward of tgcn_cheb_project_series_f32; g is the gradient of its output in the layout g_as_series names (read in place).
 *   G  (nullable, (K, S, n_vertices, T*f)):  G[k, s, i, t*f + c] = sum_h sum_m g[(s, t-h), i, m] W[k, h*f + c, m]  -- per-term input
 *      gradients for the hops on L^T, by the forward's kernel on the time-flipped transposed weight (built in the workspace)
 *   dW (nullable, (K, H*f, N)):  dW[k, h*f + c, m] = sum_{s,w,i} stack[k, s, i, (w+h)*f + c] g[(s, w), i, m]; fp32 MFMA, partial sums per
 *      row block folded in block order (deterministic).  The workspace must be 16-byte aligned. */
size_t tgcn_cheb_series_backward_workspace_bytes(int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K);
int tgcn_cheb_series_backward_f32(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                  const float* stack, const float* g, int32_t g_as_series, const float* W, float* G, float* dW,
                                  void* workspace, size_t workspace_bytes);

/* Host-only query of the launch tgcn_cheb_project_series_f32 / the input gradient of tgcn_cheb_series_backward_f32 make for H time rows of f
 * channels and N columns (forward: (H, f, N); input gradient: (H, N, K*f)); vec = 16-byte loads (f % 4 == 0 and an aligned source).
 *   hc: weight time rows per staged LDS span (hc == H: the whole horizon at once; less: the horizon in chunks); lds_bytes: dynamic LDS of
 *   the launch (above 65536: the device's opt-in limit is used; without a device that limit is 65536).
 * TGCN_ERR_UNSUPPORTED when one time row does not fit the limit: the launch would be refused with the same code. */
int tgcn_series_gemm_plan(int32_t H, int32_t f, int32_t N, int32_t vec, int32_t* hc, int32_t* lds_bytes);

/* The two entries above as a convolution over time with a window step and zero padding ("stride and padding"):
 * 0 <= pad_left, pad_right <= H-1 zero time rows in front of / behind every recording, Tp = T + pad_left + pad_right >= H,
 * nwin = (Tp - H) / stride + 1 windows, window w covering the time rows w*stride - pad_left ... + H - 1 (zeros outside 0 <= t < T):
 *   out[(s, w, i), :] = sum_k sum_{h, c} stack[k, s, i, (w*stride - pad_left + h)*f + c] . W[k, h*f + c, :] + bias
 * with out (S*nwin, n_vertices, N) or, as_series, (S, n_vertices, nwin, N).  stack stays (K, S, n_vertices, T*f): nothing is padded in memory.
 * Backward: G (nullable, (K, S, n_vertices, T*f)) is written whole -- time rows that no window covers get exact zeros, gradient that falls
 * into the padding is dropped -- by one step-1 launch of the forward's kernel per phase (t + pad_left) % stride, each over the weight time
 * rows of its phase; dW (nullable) as above, a (w, h) pair outside the recording contributing nothing.  A stride above Tp (one window) is
 * taken as Tp.  (stride, pad_left, pad_right) = (1, 0, 0) makes the launches of the entries above: bit-identical results. */
int tgcn_cheb_project_series_conv_f32(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                      const float* stack, const float* W, const float* bias, int32_t bias_kind, int32_t as_series, float* out,
                                      int32_t stride, int32_t pad_left, int32_t pad_right);
size_t tgcn_cheb_series_conv_backward_workspace_bytes(int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                                      int32_t stride, int32_t pad_left, int32_t pad_right);
int tgcn_cheb_series_conv_backward_f32(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                       const float* stack, const float* g, int32_t g_as_series, const float* W, float* G, float* dW,
                                       void* workspace, size_t workspace_bytes, int32_t stride, int32_t pad_left, int32_t pad_right);

/* tgcn_series_gemm_plan for a window step: the span of hc weight time rows holds 31 * min(stride, hc) + hc time rows (from stride >= hc on
 * only the rows that are read are staged), so a step moves ordinary shapes out of the whole-horizon regime earlier.  The padding does not
 * enter.  The forward asks with (H, f, N, stride).  The input gradient runs its phases at step 1 on g as a series of N channels; phase 0 has
 * the most weight time rows and asks with (ceil(H / stride), N, K*f, 1), the other phases with that or one row less. */
int tgcn_series_conv_plan(int32_t H, int32_t f, int32_t N, int32_t vec, int32_t stride, int32_t* hc, int32_t* lds_bytes);

/* The streaming time windows on bf16 tensors (DESIGN.md 3.10 "bf16"): ONE entry family, the strided, zero-padded geometry of the _conv
 * entries above; (stride, pad_left, pad_right) = (1, 0, 0) is the plain sliding window.
 *   stack: bf16 (K, S, n_vertices, .) with stack_ld >= T*f ELEMENTS per vertex row (the rows may carry trailing padding, e.g. up to a
 *          multiple of 8 for the 16-byte hop form; the time rows inside stay f contiguous elements); W: bf16 (K, H*f, N) in the working basis;
 *          bias: fp32 or bf16 (bias_dtype = TGCN_DTYPE_*), added in fp32; out: bf16, (S*nwin, n_vertices, N) or, as_series, (S, n_vertices,
 *          nwin, N), each element rounded once from its fp32 sum.
 * Products run on v_mfma_f32_16x16x32_bf16 with fp32 accumulators.  16-byte loads when f % 8 == 0, stack_ld % 8 == 0 and stack is 16-byte
 * aligned; element loads otherwise.
 * Backward: g bf16 in the layout g_as_series names, read in place; G (nullable) fp32 (K, S, n_vertices, T*f), written whole, one launch per
 * phase of the window step over the time-flipped transposed bf16 weight (16-byte loads of g when N % 8 == 0 and g is 16-byte aligned); dW
 * (nullable) fp32 (K, H*f, N), fp32 partials folded in block order (bit-equal across runs); W may be null when G is, stack when dW is.
 * The workspace (16-byte aligned) has the fp32 entries' size, partials capped at 256 MB.
 * tgcn_series_conv_plan_bf16: tgcn_series_conv_plan's three regimes and refusal on the bf16 span's bytes (vec: the 16-byte form, taken only
 * when f % 8 == 0); the forward asks with (H, f, N, stride), the input gradient with (ceil(H / stride), N, K*f, 1).
 * A shape the plan refuses returns TGCN_ERR_UNSUPPORTED with nothing launched. */
int tgcn_cheb_project_series_conv_bf16(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                       const void* stack, int64_t stack_ld, const void* W, const void* bias, int32_t bias_dtype,
                                       int32_t bias_kind, int32_t as_series, void* out, int32_t stride, int32_t pad_left, int32_t pad_right);
size_t tgcn_cheb_series_conv_backward_bf16_workspace_bytes(int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                                           int32_t stride, int32_t pad_left, int32_t pad_right);
int tgcn_cheb_series_conv_backward_bf16(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                        const void* stack, int64_t stack_ld, const void* g, int32_t g_as_series, const void* W, float* G,
                                        float* dW, void* workspace, size_t workspace_bytes, int32_t stride, int32_t pad_left, int32_t pad_right);
int tgcn_series_conv_plan_bf16(int32_t H, int32_t f, int32_t N, int32_t vec, int32_t stride, int32_t* hc, int32_t* lds_bytes);

/* The _conv entries (fp32 and bf16) with dilated taps ("Dilation"): tap h of a window lies h*dilation time rows after its
 * first, the window spans He = (H-1)*dilation + 1 time rows, and He takes H's place in the geometry: 0 <= pad_left, pad_right <= He-1,
 * Tp = T + pad_left + pad_right >= He, nwin = (Tp - He) / stride + 1,
 *   out[(s, w, i), :] = sum_k sum_{h, c} stack[k, s, i, (w*stride - pad_left + h*dilation)*f + c] . W[k, h*f + c, :] + bias
 * W stays (K, H*f, N), every other argument is the _conv entry's.  dilation == 1 makes the _conv entry's launches: bit-identical results;
 * so does H == 1 at any dilation >= 1 and stride == 1 (one tap has nothing to dilate, and no span would bound the dilation).
 * dilation > 1 runs at stride == 1 only (TGCN_ERR_UNSUPPORTED otherwise; dilation < 1: TGCN_ERR_INVALID): a wave owns 32 windows of one
 * phase w % dilation, which are step-1 windows of every dilation-th time row, so the launch is planned as step 1 --
 * tgcn_series_conv_plan(H, f, N, vec, 1) for the forward, (H, N, K*f, vec, 1) for the input gradient (one launch over the time-flipped weight,
 * G written whole), and the _bf16 query for the bf16 entries. */
int tgcn_cheb_project_series_dilated_f32(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                         const float* stack, const float* W, const float* bias, int32_t bias_kind, int32_t as_series, float* out,
                                         int32_t stride, int32_t pad_left, int32_t pad_right, int32_t dilation);
size_t tgcn_cheb_series_dilated_backward_workspace_bytes(int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                                         int32_t stride, int32_t pad_left, int32_t pad_right, int32_t dilation);
int tgcn_cheb_series_dilated_backward_f32(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                          const float* stack, const float* g, int32_t g_as_series, const float* W, float* G, float* dW,
                                          void* workspace, size_t workspace_bytes, int32_t stride, int32_t pad_left, int32_t pad_right,
                                          int32_t dilation);
int tgcn_cheb_project_series_dilated_bf16(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                          const void* stack, int64_t stack_ld, const void* W, const void* bias, int32_t bias_dtype,
                                          int32_t bias_kind, int32_t as_series, void* out, int32_t stride, int32_t pad_left, int32_t pad_right,
                                          int32_t dilation);
size_t tgcn_cheb_series_dilated_backward_bf16_workspace_bytes(int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                                              int32_t stride, int32_t pad_left, int32_t pad_right, int32_t dilation);
int tgcn_cheb_series_dilated_backward_bf16(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                           const void* stack, int64_t stack_ld, const void* g, int32_t g_as_series, const void* W, float* G,
                                           float* dW, void* workspace, size_t workspace_bytes, int32_t stride, int32_t pad_left, int32_t pad_right,
                                           int32_t dilation);

/* Streaming state ("Streaming state"): the causal forward of the _dilated entries on one CHUNK of a longer series.  stack
 * (K, S, n, Tc*f) (bf16: rows stack_ld elements apart) holds the hop tensors of the next Tc >= 1 time rows; ring (K, S, n, ring_ld),
 * ring_ld >= C*f, C = (H-1)*dilation, holds the C time rows before them -- slot j (elements j*f ..) the row whose absolute index is
 * j (mod C), head (0 <= head < C) the slot of the oldest; time row t < 0 of the chunk is slot (head + t + C) mod C.  out (S, n, Tc, N):
 *   out[(s, i, t), :] = sum_k sum_{h, c} row[k, s, i, t - C + h*dilation][c] . W[k, h*f + c, :] + bias
 * i.e. windows [seen, seen + Tc) of the _dilated entry on the whole series at stride 1, pads (C, 0), as_series = 1 -- bit-identical to
 * them; a zeroed ring is the causal zero padding.  Two launches on the stream: the GEMM, then the ring update, which writes rows
 * j in [max(0, Tc - C), Tc) of the stack to the slots (head + j) mod C in place; the caller then sets head = (head + Tc) mod C.
 * 16-byte accesses when the stack allows them and ring_ld is a multiple of 4 (bf16: 8) elements on a 16-byte aligned ring.
 * Planned as step 1: tgcn_series_conv_plan(H, f, N, vec, 1) / _bf16 (TGCN_ERR_UNSUPPORTED where it refuses, nothing launched).
 * TGCN_ERR_INVALID: head outside [0, C) (H == 1 keeps no ring: call the _conv entry), Tc < 1, dilation < 1, ring_ld < C*f or
 * ring_ld >= INT32_MAX, and every shape the _dilated entry refuses for a chunk of Tc rows behind C rows of padding. */
int tgcn_cheb_project_series_stream_f32(void* stream, int64_t S, int64_t n_vertices, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                        const float* stack, const float* W, const float* bias, int32_t bias_kind, float* out, float* ring,
                                        int64_t ring_ld, int32_t head, int32_t dilation);
int tgcn_cheb_project_series_stream_bf16(void* stream, int64_t S, int64_t n_vertices, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                         const void* stack, int64_t stack_ld, const void* W, const void* bias, int32_t bias_dtype,
                                         int32_t bias_kind, void* out, void* ring, int64_t ring_ld, int32_t head, int32_t dilation);

/* The stream entries with the ring's position in DEVICE memory, so that one step captured into a hipGraph can be replayed for a whole
 * recording: int64_t pos[2] = {head, seen}, owned by the caller's state next to the ring; the arguments are the entries' above with pos in
 * head's place.  Three launches, sequential on the stream (a captured step has no parallel branches): the GEMM and the ring update, which
 * both read pos[0] (one wave-uniform load per workgroup), then tgcn_series_stream_advance's kernel, pos[0] = (pos[0] + Tc) mod C and
 * pos[1] += Tc -- a launch of its own because every workgroup of the first two must have read the old head before it moves.
 * Defensive read: the host cannot check a device value without a synchronisation, so the kernels use pos[0] as head only if
 * 0 <= pos[0] < C and take 0 otherwise (one compare); no value in that memory sends a ring access out of bounds.  With a valid pos[0] the
 * results are bit-identical to the entries above at head = pos[0].
 * TGCN_ERR_INVALID: pos == NULL and everything the entries above refuse (the head rule aside); TGCN_ERR_UNSUPPORTED where the plan
 * refuses; nothing is launched in either case.
 * tgcn_series_stream_advance is the third launch alone -- for the one-tap layer, which keeps no ring (C = 0: head stays 0) and runs the
 * _conv entry, but still counts seen.  TGCN_ERR_INVALID: pos == NULL, Tc < 1, C < 0. */
int tgcn_cheb_project_series_stream_pos_f32(void* stream, int64_t S, int64_t n_vertices, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                            const float* stack, const float* W, const float* bias, int32_t bias_kind, float* out, float* ring,
                                            int64_t ring_ld, int64_t* pos, int32_t dilation);
int tgcn_cheb_project_series_stream_pos_bf16(void* stream, int64_t S, int64_t n_vertices, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                             const void* stack, int64_t stack_ld, const void* W, const void* bias, int32_t bias_dtype,
                                             int32_t bias_kind, void* out, void* ring, int64_t ring_ld, int64_t* pos, int32_t dilation);
int tgcn_series_stream_advance(void* stream, int64_t* pos, int32_t Tc, int32_t C);

/* relu + vertex max-pool as the epilogue of the streaming projection ("relu + pool epilogue"; fp32, forward only):
 *   z[.., j, ..] = max over i in [j*pool, (j+1)*pool) of relu(y[.., i, ..]),   y the output of the _conv / _dilated entry of the same arguments,
 * bit-identical to tgcn_relu_pool_f32 applied to y (members ascending, first maximum wins, NaN propagates), with y never written: a
 * workgroup owns 32 windows of four consecutive vertices and takes the max out of LDS.  pool is 2 or 4 and divides n_vertices.
 * z and idx are (S*nwin, n/pool, N) for as_series == 0 and (S, n/pool, nwin, N) otherwise; idx (one arg-max byte per element of z, what
 * tgcn_relu_pool_bwd_f32 reads) may be NULL.  Geometry (stride, pads, dilation) by the rules of the _conv / _dilated entries.
 * tgcn_series_pool_plan: tgcn_series_conv_plan's *hc and refusal -- the epilogue never changes the regime -- and *lds_bytes =
 * max(the GEMM's bytes, the scratch's 4 * 32 * (16 | 32 | 64) * 4 for N <= 16 | <= 32 | above).
 * tgcn_cheb_project_series_stream_pool_f32: the step of tgcn_cheb_project_series_stream_f32 (pos == NULL: the host's head) or of
 * tgcn_cheb_project_series_stream_pos_f32 (pos non-null: the device position, head unused, and the advance), ring update included, with
 * z (S, n/pool, Tc, N) in out's place.  H == 1 keeps no ring: the first entry on the chunk (ring, head and pos unused and not moved).
 * TGCN_ERR_INVALID before any launch: pool outside {2, 4}, n_vertices % pool != 0, a null stack, W, z (or ring for H > 1), and everything
 * the entries they extend refuse; TGCN_ERR_UNSUPPORTED where the plan refuses or a dilation meets a window step. */
int tgcn_series_pool_plan(int32_t H, int32_t f, int32_t N, int32_t vec, int32_t stride, int32_t pool, int32_t* hc, int32_t* lds_bytes);
int tgcn_cheb_project_series_pool_f32(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                      const float* stack, const float* W, const float* bias, int32_t bias_kind, int32_t as_series, float* z,
                                      uint8_t* idx, int32_t pool, int32_t stride, int32_t pad_left, int32_t pad_right, int32_t dilation);
int tgcn_cheb_project_series_stream_pool_f32(void* stream, int64_t S, int64_t n_vertices, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                             const float* stack, const float* W, const float* bias, int32_t bias_kind, float* z, int32_t pool,
                                             float* ring, int64_t ring_ld, int32_t head, int64_t* pos, int32_t dilation);

/* Dropout between relu and the pool ("dropout in the relu + pool epilogue"; fp32): the mask is a pure function of
 * (seed, element index e), never stored.  Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl increments 0x9E3779B9 / 0xBB67AE85)
 * on the counter (lo32(e >> 2), hi32(e >> 2), 0, 0) under the key (lo32(seed), hi32(seed)); element e is kept iff output word e & 3 is
 * >= thr, thr = min(floor(p * 2^32 + 0.5), 2^32 - 1); a kept value is multiplied by scale = 1 / (1 - p) (fp32), a dropped one by 0 (a
 * dropped +Inf is NaN, NaN stays NaN).  e counts the layer's output in the caller's vertex labels whatever the layout:
 * ((s * nwin + w) * n + v) * N + c for the streaming layers, (q * n + v) * N + c for the batch layers.  seed points to ONE int64 in device
 * memory, 0 <= seed < 2^62, read by the kernels: a captured step that rewrites it draws a new mask on every replay.
 * tgcn_cheb_project_series_pool_dropout_f32: tgcn_cheb_project_series_pool_f32 with t = relu(y) * mask in relu(y)'s place -- the same
 * arguments, layouts, plan (tgcn_series_pool_plan: the dropout adds no LDS) and refusals with the same codes, then seed, thr, scale.
 * z is bit-identical to tgcn_relu_dropout_pool_f32 on the unfused output; idx is the arg-max over the dropped values.  The backward is
 * tgcn_relu_pool_bwd_f32 on grad_z * scale: z > 0 implies the arg-max was kept.
 * tgcn_relu_dropout_pool_f32: tgcn_relu_pool_f32 with the mask, as its own pass over y (q, n, f) with f = nw * N columns per vertex row --
 * column cc is window cc / N, channel cc % N, e = ((q_row * nw + cc / N) * n + v) * N + cc % N: (S*nwin, n, N) with nw = 1, the
 * (S, n, nwin*N) view of a series, and the batch layers' (q, n, N).
 * tgcn_dropout_keep_u8: out[i] = 1 where element e0 + i is kept, else 0, i < count.
 * TGCN_ERR_INVALID before any launch: a null seed, a scale that is not finite or below 1, f % N != 0, e0 < 0, count < 1, and everything
 * the entries they extend refuse. */
int tgcn_cheb_project_series_pool_dropout_f32(void* stream, int64_t S, int64_t n_vertices, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                              const float* stack, const float* W, const float* bias, int32_t bias_kind, int32_t as_series, float* z,
                                              uint8_t* idx, int32_t pool, int32_t stride, int32_t pad_left, int32_t pad_right, int32_t dilation,
                                              const int64_t* seed, uint32_t thr, float scale);
int tgcn_relu_dropout_pool_f32(void* stream, const float* y, float* out, uint8_t* idx, int64_t q, int64_t n, int32_t f, int32_t pool, int32_t N,
                               const int64_t* seed, uint32_t thr, float scale);
int tgcn_dropout_keep_u8(void* stream, const int64_t* seed, int64_t e0, int64_t count, uint32_t thr, uint8_t* out);

/* Time chunks of the causal layer with a backward ("Time chunks"; fp32, step 1, the host's head): forward_series walks a
 * recording chunk by chunk through the ring in both directions, so nothing of the hop stack's whole size is ever held.
 * tgcn_cheb_project_series_stream_at_f32 is tgcn_cheb_project_series_stream_f32 writing its Tc rows into rows [out_t0, out_t0 + Tc) of
 * an output of out_T time rows, (S, n, out_T, N) for out_as_series != 0 and (S*out_T, n, N) otherwise; only the output's strides and
 * base differ, so on one stack and ring its rows and the ring afterwards are bit-identical to that entry's.  H == 1 is admitted: no ring
 * (NULL, ring_ld and head unused), one launch, nothing to update.  TGCN_ERR_INVALID: out_T < 1, out_t0 < 0, out_t0 + Tc > out_T, and
 * everything the stream entry refuses (for H == 1: the _conv entry's rules for the chunk).
 * tgcn_cheb_series_chunk_backward_f32: both gradients of the chunk's windows.  g is the WHOLE output gradient, (S, n, g_T, N) for
 * g_as_series != 0 and (S*g_T, n, N) otherwise, read in place from row g_t0 on with its own strides; 0 <= g_t0, g_t0 + Tc <= g_T.
 *   G  (K, S, n, Tc*f), non-null: rows [g_t0, g_t0 + Tc) of tgcn_cheb_series_dilated_backward_f32's G on the whole g at stride 1 and pads
 *      (C, 0), bit-identical to them -- the weight flip into the workspace and ONE launch of the sliding-window GEMM over the rows
 *      [g_t0, min(g_T, g_t0 + Tc + C)) of g; needs W (K, H*f, N).
 *   dW (K, H*f, N), non-null: the contribution of the windows that END in the chunk,
 *        dW[k][h*f + c][:] = sum_{s, i, w < Tc} row[k, s, i, w - C + h*dilation][c] . g[(s, i, g_t0 + w), :]
 *      with rows t >= 0 from stack (K, S, n, Tc*f) and rows t < 0 from the ring's slot (head + t + C) mod C, as the forward stages them;
 *      partials per row block in the workspace, folded in block order: deterministic.  Needs stack and, for H > 1, ring.
 *   ring non-null (H > 1): after both, the stream entries' ring update from stack; the caller then sets head = (head + Tc) mod C.
 * G == NULL or dW == NULL (then stack and ring may be NULL: no ring is read or moved) are the one-sided forms; both NULL is refused.
 * workspace: 16-byte aligned, tgcn_cheb_series_chunk_backward_workspace_bytes(...) bytes (0 for a shape the entry refuses).
 * TGCN_ERR_INVALID: the stream entry's rules for the chunk (head and ring_ld where a ring is given), the place of the chunk in g, a
 * missing pointer; TGCN_ERR_WORKSPACE; TGCN_ERR_UNSUPPORTED where the plan of the GEMM over g -- tgcn_series_conv_plan(H, N, K*f, vec, 1)
 * -- or a grid limit refuses.  Nothing is launched on any error; the entries do not synchronise and do not allocate. */
int tgcn_cheb_project_series_stream_at_f32(void* stream, int64_t S, int64_t n_vertices, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                           const float* stack, const float* W, const float* bias, int32_t bias_kind, float* out, int32_t out_T,
                                           int32_t out_t0, int32_t out_as_series, float* ring, int64_t ring_ld, int32_t head, int32_t dilation);
size_t tgcn_cheb_series_chunk_backward_workspace_bytes(int64_t S, int64_t n_vertices, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                                       int32_t dilation);
int tgcn_cheb_series_chunk_backward_f32(void* stream, int64_t S, int64_t n_vertices, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                        const float* stack, float* ring, int64_t ring_ld, int32_t head, const float* g, int32_t g_T,
                                        int32_t g_t0, int32_t g_as_series, const float* W, float* G, float* dW, void* workspace,
                                        size_t workspace_bytes, int32_t dilation);

/* Time chunks through the relu + dropout + pool epilogue ("Time chunks through the pooled epilogue"; fp32, step 1, the
 * host's head): the chunked walk above with the pooled epilogue in the projection's place, so neither the hop stack nor the layer's output
 * nor that output's gradient is ever held whole.
 * tgcn_cheb_project_series_stream_pool_at_f32 is the step of tgcn_cheb_project_series_stream_pool_f32 (pos == NULL) writing its Tc pooled
 * rows into rows [out_t0, out_t0 + Tc) of a whole z of out_T time rows, (S, n/pool, out_T, N) for out_as_series != 0 and
 * (S*out_T, n/pool, N) otherwise; idx (nullable) receives the arg-max bytes in the same layout and rows.  seed == NULL: no dropout (thr
 * and scale unused) -- that entry's kernels, ring update included, so on one stack and ring the rows and the ring afterwards are
 * bit-identical to it.  seed non-null: t = relu(y) * mask in relu(y)'s place by the rules of the dropout entries above, the mask's element
 * index taken at the ABSOLUTE window, e = ((s * out_T + out_t0 + w) * n + v) * N + c -- what tgcn_relu_dropout_pool_f32 gives on the
 * _stream_at entry's rows inside a whole output of out_T rows, bit for bit, whatever the chunking.  H == 1 is admitted: no ring (NULL,
 * ring_ld and head unused), the pooled forms of a whole series on the chunk, nothing to update.  The caller sets head = (head + Tc) mod C.
 * TGCN_ERR_INVALID before any launch: pool outside {2, 4}, n_vertices % pool != 0, a seed with a scale that is not finite or below 1,
 * out_T < 1, out_t0 < 0, out_t0 + Tc > out_T, a null stack, W, z (or ring for H > 1), and everything the _stream_at entry refuses;
 * TGCN_ERR_UNSUPPORTED where tgcn_series_pool_plan(H, f, N, vec, 1, pool) or a grid limit refuses.
 * tgcn_relu_pool_bwd_rows_f32: tgcn_relu_pool_bwd_f32's routing for the time rows [t0, t0 + rows) of whole pooled tensors grad_z, z, idx
 * of out_T time rows -- (S, n/pool, out_T, N) for as_series != 0 and (S*out_T, n/pool, N) otherwise -- into the dense slab grad_y of those
 * rows alone, (S, n, rows, N) or (S*rows, n, N), every element written:
 *   grad_y[s, v, r, c] = (z > 0 && idx == v % pool) ? grad_z * scale : 0      at (s, v / pool, t0 + r, c),
 * grad_z * scale one fp32 multiply (the dropout's 1 / (1 - p), or 1).  The slab is what tgcn_cheb_series_chunk_backward_f32 reads with
 * g_T = rows and g_t0 = 0.  Grid-stride with 64-bit offsets.  TGCN_ERR_INVALID: a null pointer, S, n, N < 1, pool outside [1, 255],
 * n % pool != 0, out_T < 1, t0 < 0, rows < 1, t0 + rows > out_T, a scale that is not finite.
 * Nothing is launched on any error; the entries do not synchronise and do not allocate. */
int tgcn_cheb_project_series_stream_pool_at_f32(void* stream, int64_t S, int64_t n_vertices, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                                const float* stack, const float* W, const float* bias, int32_t bias_kind, float* z, uint8_t* idx,
                                                int32_t pool, int32_t out_T, int32_t out_t0, int32_t out_as_series, float* ring, int64_t ring_ld,
                                                int32_t head, int32_t dilation, const int64_t* seed, uint32_t thr, float scale);
int tgcn_relu_pool_bwd_rows_f32(void* stream, const float* grad_z, const float* z, const uint8_t* idx, float* grad_y, int64_t S, int64_t n,
                                int32_t out_T, int32_t t0, int32_t rows, int32_t N, int32_t pool, int32_t as_series, float scale);

/* A window step on the streaming state ("Window step"): the stream entries' chunk, ring and position at dilation 1, with
 * only every stride-th window projected.  pos == NULL: head is the host's (0 <= head < C); pos non-null: the _pos entries' device position
 * {head, seen} and defensive read (the head argument is unused).  win_off (0 <= win_off < stride) is the chunk row at which the chunk's
 * first window ends -- (-seen) mod stride for a chunk that starts at absolute row seen -- m = win_off < Tc ? (Tc - win_off - 1)/stride + 1 : 0
 * windows end inside the chunk, out is (S, n, m, N), and window r ends at chunk row win_off + r*stride:
 *   out[(s, i, r), :] = sum_k sum_{h, c} row[k, s, i, win_off + r*stride - (H-1) + h][c] . W[k, h*f + c, :] + bias
 * with rows t < 0 from the ring's slot (head + t + C) mod C: the rows [(seen + win_off)/stride, ... + m) of the _conv entry on the whole
 * stack at pads (H-1, 0), as_series = 1 and the same stride, bit-identical to them.  Launches, sequential on the stream: the GEMM if
 * m > 0; the stream entries' ring update if H > 1 (the ring keeps EVERY row, not every stride-th); tgcn_series_stream_advance's kernel
 * if pos is non-null.  m == 0 admits out == NULL.  H == 1 is admitted: C = 0, ring may be NULL, no update.  stride == 1 (win_off == 0)
 * makes the launches of the entries above at dilation 1.
 * Planned with the step: tgcn_series_conv_plan(H, f, N, vec, stride) / _bf16 (TGCN_ERR_UNSUPPORTED where it refuses).
 * TGCN_ERR_INVALID: stride < 1, win_off outside [0, stride), and everything the stream entries refuse (the head rule only when pos is
 * NULL and H > 1).  Nothing is launched on either error; the entries do not synchronise and do not allocate. */
int tgcn_cheb_project_series_stream_strided_f32(void* stream, int64_t S, int64_t n_vertices, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                                const float* stack, const float* W, const float* bias, int32_t bias_kind, float* out, float* ring,
                                                int64_t ring_ld, int32_t head, int64_t* pos, int32_t stride, int32_t win_off);
int tgcn_cheb_project_series_stream_strided_bf16(void* stream, int64_t S, int64_t n_vertices, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                                                 const void* stack, int64_t stack_ld, const void* W, const void* bias, int32_t bias_dtype,
                                                 int32_t bias_kind, void* out, void* ring, int64_t ring_ld, int32_t head, int64_t* pos,
                                                 int32_t stride, int32_t win_off);

/* One streaming step in ONE launch, for operands that fit in LDS ("One launch per step"; fp32): the K - 1 hops on the
 * chunk's rows, the stream entry's projection and its ring update, out of LDS.  chunk (S, n, Tc*f) is the INPUT of the layer in the operand's
 * labels (not a hop stack: the terms are made here, mode 0 the monomials P_k = A P_{k-1}, mode 1 Chebyshev T_k = 2 A T_{k-1} - T_{k-2}); W
 * (K, H*f, N) in the basis of that mode, bias / bias_kind, out (S, n, Tc, N), ring (K, S, n, ring_ld), head and dilation as in
 * tgcn_cheb_project_series_stream_f32, and the ring after the call is the ring that entry leaves.  One workgroup per recording owns every
 * ring row of it, so no workgroup waits for another; the chunk is walked in sub-chunks of tb time rows, each an ordinary stream step, and
 * the sums (fp32 products and sums, terms ascending, (h, c) ascending within a term, bias last) are grouped as the stream entry's: equal to
 * it up to the order in which a hop adds its neighbours.  Any f, N, K >= 1 (K = 1: no hop), H >= 2, no alignment asked of any pointer.
 * pos non-null: the head is read from pos[0] on the device by the _pos entries' defensive rule (the head argument is unused), and the caller
 * follows the call with tgcn_series_stream_advance -- every workgroup has read the old head before it moves; pos is never written here.
 * tgcn_cheb_stream_small_plan answers 0 with *tb (time rows per sub-chunk), *dense (1: the dense n x (n|1) copy of the operand in LDS, 0: its
 * CSR -- the smaller of the two) and *lds_bytes, or TGCN_ERR_UNSUPPORTED where the shape does not fit: n > 1024, more than 2^20 entries,
 * operand + the mode's 2 / 3 term buffers at tb = 1 above 160 KB of LDS, or more (vertex tile, column tile) pairs than the accumulators of
 * 1024 threads hold (ceil(n/16) * ceil(N/16) > 256); TGCN_ERR_INVALID for a non-positive f, H, N, K, Tc or dilation, a mode other than 0 / 1
 * or a null result pointer.  A is square (the caller's check: tgcn_csr has no column count).
 * _f32: TGCN_ERR_INVALID for what the stream entry refuses (head outside [0, C) with pos == NULL, Tc < 1, dilation < 1, ring_ld < C*f,
 * H < 2, a null pointer, bias_kind); TGCN_ERR_UNSUPPORTED where the plan refuses; nothing is launched in either case.  One launch; the
 * entry does not synchronise and does not allocate. */
int tgcn_cheb_stream_small_plan(int64_t n, int64_t nnz, int32_t mode, int32_t f, int32_t H, int32_t N, int32_t K, int32_t Tc, int32_t dilation,
                                int32_t* tb, int32_t* dense, int32_t* lds_bytes);
int tgcn_cheb_stream_small_f32(void* stream, const tgcn_csr* A, int32_t mode, int64_t S, int32_t Tc, int32_t f, int32_t H, int32_t N, int32_t K,
                               const float* chunk, const float* W, const float* bias, int32_t bias_kind, float* out, float* ring,
                               int64_t ring_ld, int32_t head, const int64_t* pos, int32_t dilation);

/* A whole-series time-window layer in ONE launch, for operands that fit in LDS ("One launch per series"; fp32): the K - 1
 * hops and the window projection of tgcn_cheb_project_series_dilated_f32 at stride 1, out of LDS.  series (S, n, T*f) is the INPUT of the
 * layer in the operand's labels (not a hop stack: the terms are made here, mode 0 the monomials P_k = A P_{k-1}, mode 1 Chebyshev
 * T_k = 2 A T_{k-1} - T_{k-2}); W (K, H*f, N) in the basis of that mode, bias / bias_kind, as_series, out ((S, n, nwin, N) or
 * (S*nwin, n, N), nwin = T + left + right - (H-1)*dilation), the zero pads left / right and dilation as in that entry.  The grid is
 * S * ceil(nwin / tb) independent workgroups: each owns tb windows of one recording, loads the tb + (H-1)*dilation time rows they touch and
 * hops them itself, so no workgroup reads what another writes.  Sums: fp32 products and sums, terms ascending, (h, c) ascending within a
 * term, bias last -- the series entries' order, the same at every tile; equal to hops + the _dilated entry up to the order in which a hop
 * adds its neighbours.  stack non-null: the hop stack (K, S, n, T*f) the backward entries read is written too: the tiles partition the time
 * rows [0, T) of a recording, and every element is written once, by the workgroup that owns its row, from values it computed itself; NULL:
 * nothing of that size is touched.  Any f, H, N, K >= 1, no alignment asked.
 * tgcn_cheb_series_small_plan is a host query: 0 with *tb (windows per workgroup), *dense (1: the dense n x (n|1) copy of the operand in
 * LDS, 0: its CSR -- the smaller of the two) and *lds_bytes, or TGCN_ERR_UNSUPPORTED where nothing fits: n > 1024, more than 2^20 entries,
 * N > 1024, or operand + span buffers (one in mode 0, two in mode 1) at tb = 1 above 160 KB of LDS; TGCN_ERR_INVALID for a non-positive
 * n, f, H, N, K, T or dilation, a pad outside [0, (H-1)*dilation], a window longer than the padded recording, a mode other than 0 / 1 or a
 * null result pointer.  A is square (the caller's check: tgcn_csr has no column count).
 * _f32: the plan's codes, TGCN_ERR_INVALID for a null A, series, W or out, S < 1 or a bad bias_kind, TGCN_ERR_UNSUPPORTED where n*T*f,
 * n*nwin*N, K*H*f*N or the workgroup count reach 2^31; nothing is launched in any of these cases.  One launch (a grid of 2^32 threads or
 * more is issued in parts); the entry does not synchronise and does not allocate. */
int tgcn_cheb_series_small_plan(int64_t n, int64_t nnz, int32_t mode, int32_t f, int32_t H, int32_t N, int32_t K, int32_t T, int32_t left,
                                int32_t right, int32_t dilation, int32_t* tb, int32_t* dense, int32_t* lds_bytes);
int tgcn_cheb_series_small_f32(void* stream, const tgcn_csr* A, int32_t mode, int64_t S, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                               const float* series, const float* W, const float* bias, int32_t bias_kind, int32_t as_series, float* out,
                               float* stack /* nullable */, int32_t left, int32_t right, int32_t dilation);

/* tgcn_cheb_series_small_f32 with relu, an optional dropout and the max over `pool` (2 or 4) consecutive vertices as its epilogue (DESIGN.md
 * 3.10, "relu + pool in the one-launch series layer"; fp32): still ONE launch, and the layer's (S, n, nwin, N) output is never written.  The
 * four accumulator floats of a lane are four consecutive vertices from a multiple of 4 on -- one group of 4 or two pairs -- so the pool runs in
 * registers.  Per element of the unpooled output: t = acc + bias; with seed non-null t = relu(t) * m, m = scale where dropout.h's mask keeps
 * element e = ((s * nwin + w) * n + v) * N + c (Philox4x32-10 on e >> 2 under *seed, word e & 3 >= thr -- tgcn_dropout_keep_u8 reproduces it)
 * and 0 elsewhere; then tgcn_relu_pool_f32's rules: members ascending, the first maximum wins, a NaN wins over a number,
 * z = best > 0 ? best : (NaN ? NaN : 0).  z is (S, n/pool, nwin, N) as_series, else (S*nwin, n/pool, N); idx (nullable) holds the arg-max
 * member of every element in z's layout, what tgcn_relu_pool_bwd_f32 reads.  z and idx have the bits of tgcn_relu_pool_f32 /
 * tgcn_relu_dropout_pool_f32 on tgcn_cheb_series_small_f32's output.  stack (nullable) as there.  seed NULL: no dropout, thr and scale unread.
 * The plan is tgcn_cheb_series_small_plan: the pool adds no LDS and no threads.
 * Codes: tgcn_cheb_series_small_f32's own, then TGCN_ERR_INVALID for a pool outside {2, 4}, n % pool != 0, and a non-null seed with a scale
 * that is not finite and >= 1; nothing is launched and no pointer is read in any of these cases.  The grid is issued in parts as there;
 * the entry does not synchronise and does not allocate. */
int tgcn_cheb_series_small_pool_f32(void* stream, const tgcn_csr* A, int32_t mode, int64_t S, int32_t T, int32_t f, int32_t H, int32_t N, int32_t K,
                                    const float* series, const float* W, const float* bias, int32_t bias_kind, int32_t as_series, float* z,
                                    uint8_t* idx /* nullable */, int32_t pool, float* stack /* nullable */, int32_t left, int32_t right,
                                    int32_t dilation, const int64_t* seed /* NULL: no dropout */, uint32_t thr, float scale);

/* Weight gradient of the projection (backward of gcn.py:39,113,194 w.r.t. weight):
 *   dW[t*Kc + c, n] = sum_m A_t[m, c] * G[m, n]
 * A_t as in tgcn_cheb_project_f32 (host arrays of nterms <= 32 pointers / strides), G: M x N with row stride ldg,
 * dW: (nterms*Kc) x N contiguous.  fp32 MFMA, two-stage reduction in fixed order (deterministic). */
size_t tgcn_cheb_wgrad_workspace_bytes(int64_t M, int32_t Kc, int32_t N, int32_t nterms);
int tgcn_cheb_wgrad_f32(void* stream, int64_t M, int32_t Kc, int32_t N, int32_t nterms, const float* const* a,
                        const int64_t* lda, const float* G, int64_t ldg, float* dW, void* workspace, size_t workspace_bytes);

/* tgcn_cheb_project_f32's contraction on bf16 terms a[t] and a bf16 W ((nterms*Kc) x N): products on the bf16 matrix pipe, fp32 sums,
 * bias (bias_dtype: TGCN_DTYPE_F32 or TGCN_DTYPE_BF16) added in fp32 to the first bias_cols columns (<= 0: all N; a per-vertex bias row
 * then has bias_cols elements), accumulate adds the existing output; out (out_dtype) is fp32, or rounded once to bf16.  interleave as in
 * tgcn_cheb_project_f32; k past nterms*Kc in the last 32-wide step reads zeros. */
int tgcn_cheb_project_bf16(void* stream, int64_t M, int32_t Kc, int32_t N, int32_t nterms, const void* const* a, const int64_t* lda,
                           const void* W, const void* bias, int32_t bias_kind, int32_t bias_dtype, int32_t bias_cols, int64_t n_vertices,
                           int64_t interleave, int32_t accumulate, void* out, int64_t ldo, int32_t out_dtype);

/* tgcn_cheb_project_bf16's contraction through tgcn_cheb_project_mapped_f32's ROW MAP at interleave = 1 (the building block of the compacted
 * bf16 layers): tile row m is the caller's vertex rowmap[m] (int32 device array of M entries, each < n_vertices) -- its output
 * row, its bias row, and its row in every term t whose bit t is set in `mapped_terms`; the other terms are read at row m.  nbatch samples share
 * the tile rows (grid.z): sample b reads term t at a[t] + b * a_bs[t] ELEMENTS and writes out + b * out_bs elements.  a_bs: HOST array of
 * nterms strides (nullable for nbatch = 1).  The bias (fp32 or bf16, all N columns) is added in fp32; out is fp32, or rounded once to bf16;
 * rows that the map does not name are not touched.  Row offsets are 64-bit after the map.  16-byte A loads when every a[t] is 16-byte
 * aligned and Kc, lda[t] and a_bs[t] are multiples of 8, element loads otherwise.  A mapped row holds the bits tgcn_cheb_project_bf16 gives
 * the same row of explicitly gathered terms.  TGCN_ERR_INVALID for a null rowmap, nbatch < 1, nbatch > 1 without a_bs, M <= 0 (an empty map
 * is the caller's case) or what tgcn_cheb_project_bf16 refuses; nothing is launched then. */
int tgcn_cheb_project_mapped_bf16(void* stream, int64_t M, int32_t Kc, int32_t N, int32_t nterms, const void* const* a, const int64_t* lda,
                                  const void* W, const void* bias, int32_t bias_kind, int32_t bias_dtype, int64_t n_vertices, const int32_t* rowmap,
                                  uint32_t mapped_terms, int32_t nbatch, const int64_t* a_bs, int64_t out_bs, void* out, int64_t ldo,
                                  int32_t out_dtype);

/* tgcn_cheb_wgrad_f32 on bf16 A_t and G (fp32 dW and partials): bf16 matrix pipe (exact products), the same two-stage reduction in fixed
 * order (deterministic); workspace: tgcn_cheb_wgrad_workspace_bytes. */
int tgcn_cheb_wgrad_bf16(void* stream, int64_t M, int32_t Kc, int32_t N, int32_t nterms, const void* const* a, const int64_t* lda,
                         const void* G, int64_t ldg, float* dW, void* workspace, size_t workspace_bytes);

/* (Q, n, C) -> (n, Q, C) re-layout so that short per-sample rows become one long row per vertex (LDS-tiled transpose for C <= 32, a
 * coalesced row copy for wider rows). */
int tgcn_relayout_qnc_to_nqc_f32(void* stream, const float* in, float* out, int64_t Q, int64_t n, int32_t C);

/* Whole layer forward: K-1 hops + projection, enqueued on `stream` (capturable in a hipGraph).
 *   mode 0 "reference_power": W must be the monomial-folded weight (see tgcn_amd/functional.py);
 *          out = sum_j (L^j x) W_j + bias          (TGCNCheb / TGCNCheb_H / GCNCheb)
 *   mode 1 "chebyshev": out = sum_k T_k(L) x W_k + bias   (ChebConv / ChebTimeConv)
 * x: (q, n, C) contiguous, C = H*f; W: (K*C) x N; out: (q, n, N) contiguous.
 * layout 0: hops run on the (q, n, C) layout as is; layout 1: x is first re-laid to (n, q*C).
 * q_chunk: samples per pass (layout 0 only; 0 = all).  Workspace: tgcn_cheb_forward_workspace_bytes. */
size_t tgcn_cheb_forward_workspace_bytes(const tgcn_csr_sched* sched, int32_t K, int64_t q, int64_t n, int32_t C,
                                         int32_t layout, int64_t q_chunk);
int tgcn_cheb_forward_f32(void* stream, const tgcn_csr* A, const tgcn_csr_sched* sched, int32_t mode, int32_t K,
                          int64_t q, int64_t n, int32_t C, int32_t N, const float* x, const float* W,
                          const float* bias, int32_t bias_kind, float* out, int32_t layout, int64_t q_chunk,
                          void* workspace, size_t workspace_bytes);

/* The same layer (mode 0 only) for operands with structurally EMPTY rows (R-MAT: 5.27 M of 10 M vertices; the isolated
 * fake vertices the reference's coarsening pads its graphs with, gcn/coarsening.py:167-217).  For such a vertex i every hop
 * tensor row P_k[i], k >= 1, is zero, so out[i] = x[i] W_0 + bias[i]; the hop tensors are kept for the n_c vertices that do
 * have entries only (compact ids = rank among them):
 *   A_first  n_c rows, columns in the caller's labels (hop 1 gathers from x);  A_rest  the same rows and entry order with
 *            columns in compact ids, entries whose column is an empty vertex pointing at the zero row n_c  (hops 2..K-1);
 *   rows[n_c] / empty_rows[n_empty]  caller's label of every compact / empty row, ascending;  sched: shared by both operands.
 * The projection reads x, bias and writes out through the row maps; hop tensors, hop writes and four of the five projection
 * terms shrink by n_empty / n.  Bitwise equal to tgcn_cheb_forward_f32 (layout 0) on the same operand.  K >= 2. */
size_t tgcn_cheb_forward_compact_workspace_bytes(const tgcn_csr_sched* sched, int32_t K, int64_t q, int64_t n_c, int32_t C,
                                                 int64_t q_chunk);
int tgcn_cheb_forward_compact_f32(void* stream, const tgcn_csr* A_first, const tgcn_csr* A_rest, const tgcn_csr_sched* sched,
                                  int32_t K, int64_t q, int64_t n, int32_t C, int32_t N, const float* x, const float* W,
                                  const float* bias, int32_t bias_kind, float* out, const int32_t* rows, const int32_t* empty_rows,
                                  int64_t n_empty, int64_t q_chunk, void* workspace, size_t workspace_bytes);

/* The compacted layer in general form (ABI v6): BOTH recurrences, and optionally the hop tensors handed back to the caller.
 *   mode 0  as tgcn_cheb_forward_compact_f32 (which is this function with mode 0, W_left = NULL, keep_terms = NULL).
 *   mode 1  true Chebyshev recurrence (ChebConv / ChebTimeConv, tgcn/nn/gcn.py:420-432, :519-528) on compact hop tensors: the kept
 *           vertices must be CLOSED -- every vertex with entries and every vertex an entry points at -- so that a left-out vertex is
 *           isolated and T_k[i] = x[i], 0, -x[i], 0, ...: out[i] = x[i] W_left + bias with W_left = W_0 - W_2 + W_4 - ... (C x N, the
 *           caller folds it: tgcn_fold_weight_f32 with the sign column).  T_0 = the kept rows of x (packed by the driver), T_1 = A_rest T_0,
 *           T_k = 2 A_rest T_{k-1} - T_{k-2}; A_first is not used.  W: (K*C) x N in the reference basis.
 *   W_left  (nullable for mode 0: the first C rows of W, i.e. W'_0)  the C x N matrix of the left-out vertices.
 *   keep_terms (nullable)  caller memory for the hop tensors, [T][q][n_c + 1][C] floats contiguous, T = K-1 (mode 0: terms 1..K-1) or
 *           K (mode 1: terms 0..K-1); row n_c of every sample is zeroed by the driver.  They are exactly the basis the weight gradient
 *           contracts with g (the training forward keeps them instead of recomputing K-1 hops in backward); all q samples are then one
 *           pass and the workspace holds the long-row scratch only.
 * One C call per layer forward replaces the host-side pipeline of K hops + 2 projections (functional.compact_forward before round 5). */
size_t tgcn_cheb_compact_layer_workspace_bytes(const tgcn_csr_sched* sched, int32_t mode, int32_t K, int64_t q, int64_t n_c, int32_t C,
                                               int64_t q_chunk, int32_t keep_terms);
int tgcn_cheb_compact_layer_f32(void* stream, const tgcn_csr* A_first, const tgcn_csr* A_rest, const tgcn_csr_sched* sched, int32_t mode,
                                int32_t K, int64_t q, int64_t n, int32_t C, int32_t N, const float* x, const float* W, const float* W_left,
                                const float* bias, int32_t bias_kind, float* out, const int32_t* rows, const int32_t* empty_rows,
                                int64_t n_empty, int64_t q_chunk, float* keep_terms, void* workspace,
                                size_t workspace_bytes);

/* "Project first" form of the same layer for wide inputs and narrow outputs (N well below C = H*f, e.g.
 * TGCNCheb_H(L, 1, 32, K, 1200)): Z = x . Wcat for all K terms in ONE projection (Wcat: C x (K*N), column block j =
 * W_j, folded for mode 0), then the recursion runs on the (q, n, N) results -- Horner  Y_j = Z_j + L Y_{j+1}  for
 * mode 0, Clenshaw for mode 1 -- so the K-1 hops move N instead of C floats per row.  Same result as
 * tgcn_cheb_forward_f32 up to fp32 re-association.  `sched` must be the schedule for rows of N floats. */
size_t tgcn_cheb_forward_pf_workspace_bytes(const tgcn_csr_sched* sched, int32_t K, int64_t q, int64_t n, int32_t N);
int tgcn_cheb_forward_pf_f32(void* stream, const tgcn_csr* A, const tgcn_csr_sched* sched, int32_t mode, int32_t K, int64_t q,
                             int64_t n, int32_t C, int32_t N, const float* x, const float* Wcat, const float* bias,
                             int32_t bias_kind, float* out, void* workspace, size_t workspace_bytes);

/* The first step of that form on its own (ABI v7): Z[b, r(m), 0:K*N] = x[b, m, 0:C] . Wcat, bias added to the first N columns (Z_0).
 * x: (q, rows, C) contiguous; Z: (q, rows, K*N) contiguous; bias: [N] (kind 1) or [rows, N] (kind 2), read at the OUTPUT row.
 * rowmap (nullable, device, int32[rows]): output row r(m) = rowmap[m] -- a vertex shard keeps its rows in the order
 * [interior | boundary] and writes Z in that order while reading x in the caller's.  The caller then runs the Horner / Clenshaw
 * recursion itself with tgcn_csr_hop2_f32 on strided views of Z: the vertex-sharded layer exchanges the cut rows of every
 * intermediate result between its hops (tgcn_amd/dist.py; reference call shape examples/pytorch_based/pytorch_hcp_tgcn.py:103-104). */
int tgcn_cheb_project_first_f32(void* stream, int64_t q, int64_t rows, int32_t C, int32_t K, int32_t N, const float* x, const float* Wcat,
                                const float* bias, int32_t bias_kind, const int32_t* rowmap, float* Z);

/* Small graphs (n <= 1024, C <= 128, CSR + activations fit in 160 KB of LDS -- the reference's own MNIST / coarsened
 * graphs): the whole layer in ONE launch, recursion run on the output side in LDS (Horner for mode 0, Clenshaw for
 * mode 1).  W: (K, C, N) contiguous; `fold` (nullable, device, K x K): the reference_power -> monomial fold matrix,
 * applied while the weight is staged so the caller passes the layer's raw weight.
 * tgcn_cheb_forward_small_supported returns the channel tile (16 / 8) or 0 when the shape does not fit.
 * Operands that store at least a quarter of their entries (n <= 256, C <= 32: the 148-parcel DTI graph of load/res) run
 * the same recursion on the matrix pipe, L held as A-fragments in registers: exact fp32 (v_mfma_f32_16x16x4_f32), or -- when
 * the batch fills the chip -- the three-way bf16 split of the projection kernels (fp32-accurate, 2.7x fewer MFMA cycles);
 * tgcn_set_tuning("small_dense", 0) keeps them on the vector-ALU kernel. */
int tgcn_cheb_forward_small_supported(int64_t n, int64_t nnz, int32_t C, int32_t mode);   /* counts on A->dense for dense operands */
int tgcn_cheb_forward_small_pool_supported(int64_t n, int64_t nnz, int32_t C, int32_t mode);   /* ... with the fused relu + pool epilogue */
int tgcn_cheb_forward_small_f32(void* stream, const tgcn_csr* A, int32_t mode, int32_t K, int64_t q, int32_t C, int32_t N,
                                const float* x, const float* W, const float* fold, const float* bias, int32_t bias_kind,
                                float* out);

/* Backward of the same shapes.  The input gradient is the forward kernel itself on the transposed operand
 * (dx = sum_j (L^T)^j g W_j^T: call tgcn_cheb_forward_small_f32 with A = L^T, x = g, W = the (K, N, C) transposed
 * working-basis weight, no bias).  The weight gradient needs the basis autograd would recompute through
 * _chebyshev / _time_chebyshev (gcn.py:52-79,126-154,208-237; true recurrence gcn.py:420-432,519-528):
 * tgcn_cheb_basis_small_f32 writes terms
 * k = 1 .. K-1 of the (K, q, n, C) stack in ONE launch (mode 0: monomials L^k x, the basis of the folded weight;
 * mode 1: Chebyshev T_k x); term 0 is x itself and is not copied.  Feed the terms to tgcn_cheb_wgrad_f32.
 * _supported returns the channel tile (16 / 8 / 4) or 0 when the operand does not fit in LDS. */
int tgcn_cheb_basis_small_supported(int64_t n, int64_t nnz, int32_t C, int32_t mode);
int tgcn_cheb_basis_small_f32(void* stream, const tgcn_csr* A, int32_t mode, int32_t K, int64_t q, int32_t C,
                              const float* x, float* stack);

/* Host query (ABI 8, additive): the kernel and launch configuration that tgcn_cheb_forward_small_pool_f32 (basis = 0; pool as passed
 * there, 0 for tgcn_cheb_forward_small_f32) or tgcn_cheb_basis_small_f32 (basis != 0; N and pool are not read) takes for an operand of n
 * vertices and nnz entries (has_dense_copy: tgcn_csr.dense is non-null), input rows of C floats, N output channels and a batch of q.  The
 * launch entries get their configuration from this very function, so what it reports is what runs; it honours the small_dense and
 * small_narrow tuning switches as they do.  Nothing is launched.
 *   form       0 small_forward_kernel (recursion on the output side), 1 small_narrow_kernel (C <= 4, recursion on the input side),
 *              2 small_basis_kernel, 3 fp32 matrix pipe (small_dense_kernel), 4 bf16x3 matrix pipe (small_dense_x3_kernel)
 *   tile       channels per workgroup: NTC (form 0), NT (form 1), CT (form 2), 16 (forms 3, 4)
 *   cp         floats of the input row a thread of form 0 keeps in registers (4 / 16 / 32); 0 for the other forms
 *   spw        samples per workgroup (forms 3, 4: their S); the last workgroup has q % spw live samples when that is not 0
 *   dense_lds  1: the operand lies in LDS as a dense n x (n|1) matrix, 0: as its CSR (forms 3, 4: 0, L is held in registers)
 *   threads, lds_bytes, grid_x, grid_y   the launch
 * Returns 0, or the code the launch entry returns for the same arguments: TGCN_ERR_INVALID for q < 1, N < 1 (forward), C < 1 (basis), a
 * pool outside [0, 255] or one that does not divide n, or a null plan; TGCN_ERR_UNSUPPORTED where the operand and buffers do not fit
 * (n > 1024, more than 2^20 entries, C > 128 in the forward, above 160 KB of LDS, a mode other than 0 / 1) or the grid is too large. */
typedef struct tgcn_small_plan {
  int32_t form, tile, cp, spw, dense_lds, threads, lds_bytes, grid_x, grid_y;
} tgcn_small_plan;
int tgcn_cheb_small_plan(int64_t n, int64_t nnz, int32_t has_dense_copy, int32_t mode, int32_t C, int32_t N, int64_t q, int32_t pool,
                         int32_t basis, tgcn_small_plan* plan);

/* Fused epilogue of the callers' pattern  x = gcn_pool_4(F.relu(layer(x)))  (examples/pytorch_based/
 * pytorch_hcp_tgcn.py:134-141): out (q, n/pool, N) = max over `pool` consecutive vertices of
 * relu(layer output); pool_idx (nullable, uint8) receives the arg-max offset for the backward.
 * _small_pool: inside the one-launch small-graph kernel (the layer output never reaches HBM);
 * tgcn_relu_pool_f32 / _bwd: the same epilogue as its own pass for shapes the small-graph kernel does not take. */
int tgcn_cheb_forward_small_pool_f32(void* stream, const tgcn_csr* A, int32_t mode, int32_t K, int64_t q, int32_t C, int32_t N,
                                     const float* x, const float* W, const float* fold, const float* bias, int32_t bias_kind,
                                     int32_t relu, int32_t pool, float* out, uint8_t* pool_idx);
int tgcn_relu_pool_f32(void* stream, const float* x, float* out, uint8_t* idx, int64_t q, int64_t n, int32_t f, int32_t p);

/* The layer of tgcn_cheb_forward_f32 followed by relu + max over `pool` consecutive vertices for graphs that do NOT fit in LDS:
 * out (q, n/pool, N), pool_idx (nullable) as above.  On the (q, n, C) layout with up to 32 terms the epilogue runs inside the projection
 * kernel -- N <= 64 output columns: bias, relu and the max over 2 / 4 / 8 / 16 rows of the finished tile in the wave's LDS scratch;
 * N >= 96 on the bf16x3 path (ABI v7): groups of 2 / 4 rows folded in registers, a lane's four accumulators of a column being four
 * consecutive rows -- so the (q, n, N) layer output is never written; other shapes (the vertex-major layout 1 of rows shorter than 32
 * floats, groups of 8 / 16 with wide outputs) run the layer into workspace scratch followed by tgcn_relu_pool_f32: measured 0 - 1.3 % of the
 * fused call on the layout-1 shapes of the reference's HCP model at mesh size (profiles/r06_pool_epilogue_cost.jsonl), final as it is
 * (the workspace query accounts for it; it returns 0 only for invalid arguments -- a K = 1 layer on a schedule without partial rows has
 * a base figure of 0 and still gets its output scratch).  pool = 1: relu only.
 * Alignment: the fused epilogue needs `out` and `bias` 16-byte aligned and `pool_idx` 4-byte aligned.  The query decides fused vs two-pass
 * from the shape alone; a call with a fusable shape and a misaligned pointer takes the two-pass form when the workspace also holds
 * q*n*N floats of scratch behind the queried size, and fails with TGCN_ERR_INVALID (message names the pointers) otherwise. */
size_t tgcn_cheb_forward_pool_workspace_bytes(const tgcn_csr_sched* sched, int32_t K, int64_t q, int64_t n, int32_t C, int32_t N,
                                              int32_t layout, int64_t q_chunk, int32_t pool);
int tgcn_cheb_forward_pool_f32(void* stream, const tgcn_csr* A, const tgcn_csr_sched* sched, int32_t mode, int32_t K, int64_t q,
                               int64_t n, int32_t C, int32_t N, const float* x, const float* W, const float* bias, int32_t bias_kind,
                               int32_t pool, float* out, uint8_t* pool_idx, int32_t layout, int64_t q_chunk, void* workspace,
                               size_t workspace_bytes);
int tgcn_relu_pool_bwd_f32(void* stream, const float* grad_z, const float* z, const uint8_t* idx, float* grad_y, int64_t q,
                           int64_t n, int32_t f, int32_t p);

/* Gradient of a hop w.r.t. the VALUES of its sparse operand (ABI v5): the sampled dense-dense product over the stored pattern
 *   dval[e] (+)= alpha * sum_b sum_c rows[b, row(e), c] * cols[b, col(e), c]      for every stored entry e, in CSR order
 * -- for S = L X: dL/dval_e = <dL/dS[row(e)], X[col(e)]>.  What makes `edge_weight` of ChebConv / ChebTimeConv and `value` of spmm* learnable as
 * in the reference, whose gather / scale / scatter_add form is differentiable in them (tgcn/nn/gcn.py:296-308, 413, 510).  rows: (nb, A->n, C),
 * cols: (nb, n_cols, C); one lane group per entry, fixed summation order (no atomics); accumulate != 0 adds to dval. */
int tgcn_csr_sddmm_f32(void* stream, const tgcn_csr* A, int64_t n_cols, int32_t nb, int32_t C, const tgcn_dense* rows, const tgcn_dense* cols,
                       float alpha, float* dval, int32_t accumulate);

/* Vertex sharding (replaces nn.DataParallel's batch split, examples/pytorch_based/pytorch_hcp_tgcn.py:270-273):
 * out[i, 0:C] = src[idx[i], 0:C] -- the rows of a hop tensor that a neighbouring shard needs, packed into one message.
 * idx: int64 device array; src rows ld_src floats apart; out contiguous. */
int tgcn_pack_rows_f32(void* stream, const float* src, int64_t ld_src, const int64_t* idx, int64_t nrows, int32_t C, float* out);
/* The same on 2-byte elements (bf16 rows: the kept rows of the output gradient of a compacted bf16 layer): ld_src and C in elements; 16-byte
 * pieces when C and ld_src are multiples of 8 and src and out are 16-byte aligned, element by element otherwise.  Values move unchanged. */
int tgcn_pack_rows_bf16(void* stream, const void* src, int64_t ld_src, const int64_t* idx, int64_t nrows, int32_t C, void* out);

/* gcn_pool / gcn_pool_4 (gcn.py:246-255): max over p consecutive vertices; idx (nullable) receives the
 * arg-max offset 0..p-1 for the backward. */
int tgcn_pool_max_f32(void* stream, const float* x, float* out, int32_t* idx, int64_t q, int64_t n, int32_t f,
                      int32_t p);
int tgcn_pool_max_bwd_f32(void* stream, const float* grad_out, const int32_t* idx, float* grad_in, int64_t q,
                          int64_t n, int32_t f, int32_t p);

#ifdef __cplusplus
}
#endif
#endif /* TGCN_HIP_H */
