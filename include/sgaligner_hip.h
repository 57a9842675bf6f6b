/* sgaligner_hip.h -- C ABI of libsga_hip.so (sgaligner_amd/csrc), the MI355X (gfx950) implementation of
 * SGAligner's node-embedding + matching hot path.
 *
 * The reference (sayands/sgaligner) is pure Python and has no FFI; each entry point below states the
 * reference code it replaces (paths relative to the reference repository root).  A reference-side caller
 * binds these with ctypes (INTEGRATION.md shows the stub); sgaligner_amd/_lib.py is that binding.
 *
 * Conventions
 *   - plain device pointers + sizes; the library never allocates, frees or retains memory;
 *   - all matrices row-major fp32 unless stated, base pointers 16-byte aligned;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - return 0 on success, non-zero on failure with the message available from sga_last_error()
 *     (thread-local); argument errors are detected before any launch.
 */
#ifndef SGALIGNER_HIP_H
#define SGALIGNER_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int sga_version(void);                 /* 100 * major + minor */
const char* sga_last_error(void);
int sga_device_cus(void);
/* The library is STATELESS (SURVEY 8(b) "Threading"): no entry point reads or writes a process-global setting.  Which arithmetic a
 * call uses is either in its name (sga_loss_multi_sums = exact fp32 MFMA, _centred = the same over centred tables, _bf16x6 = three exact
 * bf16 planes, *_f16 = fp16 inputs for wide tables) or an explicit argument (sga_pointnet_fwd_ws: mode).  The policy --
 * which of them a training step calls -- lives in the caller (sgaligner_amd.ops.set_mfma_mode, SGA_MFMA_MODE). */

/* ---- PointNet object encoder ------------------------------------------------------------------------
 * replaces PointNetfeat.forward, src/aligner/networks/pointnet.py:120-175 (called sg_aligner.py:115):
 *   y[t,c] = max_p relu(W3 relu(W2 relu(W1 x[t,p] + b1) + b2) + b3)[c]      (BN outputs are discarded there)
 * x [T,P,3] (data_dict['tot_obj_pts'] layout), w1 [64,3], w2 [128,64], w3 [C3,128], y [T,C3],
 * argmax [T,C3] int32 (first arg-max point per channel; NULL to skip).  C3 in {64,128,256}. */
int sga_pointnet_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                     const float* w3, const float* b3, float* y, int32_t* argmax, int T, int P, int C3,
                     void* stream);
/* Same, with a caller-owned workspace of sga_pointnet_fwd_ws_bytes(T, C3) bytes (the partials buffer): when the batch has few objects of
 * more than one 32-point tile (the reference's own batch sizes, single-pair inference: T < 4 x CUs and P > 32) every object is split over
 * the 8 waves of a workgroup and the partial (max, arg-max) pairs are folded by a second small kernel -- identical results, per-object
 * latency / 8.  workspace may be NULL (then this is sga_pointnet_fwd).  Which form a call takes: sga_pointnet_plan below. */
size_t sga_pointnet_fwd_ws_bytes(int T, int C3);
/* mode: the forward's arithmetic.  0 = exact fp32 on v_mfma_f32_32x32x2_f32 (sga_pointnet_fwd is this); 4 = every fp32 operand as THREE exact
 * bf16 terms (8 + 8 + 8 significand bits, fp32's exponent range: the value itself), six bf16 MFMAs per product into fp32 accumulators --
 * fp32 arithmetic on the bf16 matrix pipe, as the default loss sweeps (sga_loss_multi_*_bf16x6), in both launch forms (identical bits);
 * with C3 = 256, a call that is not split (T >= 4 x CUs, or P <= 32, or a workspace smaller than the partials buffer) and a workspace of
 * >= sga_pointnet_fwd_lg_ws_bytes() = 81 920 bytes, the kernel keeps the l planes of W2 / W3 there and one workgroup serves whole objects
 * (1.15 x faster).  Any workspace that large will do: a partials buffer offered for a call of P <= 32 serves as that scratch.
 * (pointnet.py:140-161) */
size_t sga_pointnet_fwd_lg_ws_bytes(void);
int sga_pointnet_fwd_ws(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                        const float* w3, const float* b3, float* y, int32_t* argmax, int T, int P, int C3,
                        void* workspace, size_t ws_bytes, int mode, void* stream);
/* The forward in mode 0 (exact fp32) or 4 (three exact bf16 planes) that ALSO delivers the side effect of the reference's training forward: its three BatchNorm calls discard
 * their output but fold the batch statistics of the pre-ReLU conv outputs over all T*P points into running_mean / running_var
 * (pointnet.py:141-142,154-155,158-159).  The sums are taken inside the forward kernel (no second pass over the activations) and folded in
 * a fixed order.  bn_sums, 265 + 2 C3 doubles:
 *   [0, 9)            sum over the points of x0, x1, x2, x0x0, x0x1, x0x2, x1x1, x1x2, x2x2   (z1 = W1 x + b1 is affine in x: the caller
 *                     forms mean and variance of the 64 channels from these moments)
 *   [9, 137)          sum z2[c]         [137, 265)          sum z2[c]^2        z2 = W2 relu(z1) + b2
 *   [265, 265 + C3)   sum u[c]          [265 + C3, + 2 C3)  sum u[c]^2         u = z3 - b3 = W3 relu(z2)
 * bn_workspace: sga_pointnet_fwd_bn_ws_bytes(T, C3) bytes, caller-owned.  workspace / ws_bytes as in sga_pointnet_fwd_ws (may be NULL).
 * sga_pointnet_fwd_bn_ws_bytes bounds what every launch form zeroes there (a form that would need more is refused, SGA_ERR_WORKSPACE, before
 * anything is written). */
size_t sga_pointnet_fwd_bn_ws_bytes(int T, int C3);
int sga_pointnet_fwd_bn(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                        const float* w3, const float* b3, float* y, int32_t* argmax, int T, int P, int C3,
                        void* workspace, size_t ws_bytes, void* bn_workspace, size_t bn_ws_bytes, double* bn_sums, int mode, void* stream);
/* autograd of the above wrt the six parameters (sparse through the max-pool: pointnet.py:140-161 through the arg-max points); gy [T,C3]; C3 == 256.
 * mode: the arithmetic of the three winner-row GEMMs (Z2 recomputation, dH1 = dZ2 W2, gW2 += dZ2^T H1) -- 0 = fp32 MFMA, 4 = three exact bf16
 * planes, six bf16 MFMAs per product into fp32 accumulators (as sga_pointnet_fwd_ws mode 4).  Everything else is fp32 VALU in both. */
int sga_pointnet_bwd(const float* x, const int32_t* argmax, const float* y, const float* gy, const float* w1,
                     const float* b1, const float* w2, const float* b2, const float* w3, float* gw1, float* gb1,
                     float* gw2, float* gb2, float* gw3, float* gb3, int T, int P, int C3, int mode, void* stream);
/* Which launch form a PointNet call takes -- the launcher's own decision (every condition that chooses a kernel, a grid or a size is in
 * this one function), for tests that must know what they ran.  Host only: with ncu > 0 (the CU count to plan for) no device is touched;
 * ncu <= 0 asks the current device.  pass: sga_pointnet_pass (sga_pointnet_fwd / _fwd_ws, sga_pointnet_fwd_bn, sga_pointnet_bwd); ws_bytes:
 * the bytes of `workspace` the call would offer (0 for none, and for the backward).  plan receives SGA_POINTNET_PLAN_FIELDS int32 (NULL: only
 * the arguments are checked):
 *   [0] form (sga_pointnet_form)              [1] workgroups of the main kernel          [2] its dynamic LDS bytes
 *   [3] what `workspace` holds (sga_pointnet_ws_use)                                     [4] the bytes of it that are used
 *   [5] bytes of bn_workspace zeroed before the launch (forward with BatchNorm sums only; otherwise 0)
 *   workgroups of the auxiliary launches, 0 = not launched, in launch order around the main kernel:
 *   [6] l-plane preparation (before)          [7] combine of the split forms' partials   [8] point moments   [9] BatchNorm reduce
 * Bad arguments are refused as the entry points refuse them: the message is set, the form is SGA_POINTNET_REFUSED and SGA_ERR_ARG returned. */
enum sga_pointnet_pass { SGA_POINTNET_FWD = 0, SGA_POINTNET_FWD_BN, SGA_POINTNET_BWD };
enum sga_pointnet_ws_use { SGA_POINTNET_WS_NONE = 0, SGA_POINTNET_WS_PARTIALS, SGA_POINTNET_WS_LG };
enum sga_pointnet_form {
    SGA_POINTNET_EMPTY = 0,       /* T == 0: nothing is launched (the backward still zeroes the gradients) */
    SGA_POINTNET_F32_WAVE,        /* exact fp32, one wave per object */
    SGA_POINTNET_F32_SPLIT,       /* exact fp32, one object per workgroup at a time, then the combine kernel */
    SGA_POINTNET_P3,              /* three planes, one wave per object; at C3 = 256 two half-workgroups share an object */
    SGA_POINTNET_P3_SPLIT,        /* three planes, split, then the combine kernel */
    SGA_POINTNET_P3_LG,           /* three planes, C3 = 256, the l planes of W2 / W3 in `workspace` */
    SGA_POINTNET_BWD_F32,         /* backward, fp32 MFMA: pairs of workgroups */
    SGA_POINTNET_BWD_P3,          /* backward, three planes: quadruples of workgroups */
    SGA_POINTNET_REFUSED
};
#define SGA_POINTNET_PLAN_FIELDS 10
int sga_pointnet_plan(int pass, int T, int P, int C3, int mode, size_t ws_bytes, int ncu, int32_t* plan);

/* ---- dense layers -----------------------------------------------------------------------------------
 * C[M,N] (+)= op(A)[M,K] op(B)[K,N] (+ bias[N]);  transX = 0: X stored [rows][K]..., see gemm.hip.
 * replaces nn.Linear fwd/bwd of object_embedding / structure_embedding / meta_embedding_rel / _attr
 * (src/aligner/sg_aligner.py:112,116,119,122) and the dS*E products of the loss backward.
 * a_is_f64 != 0: A is float64 (the collated bag-of-words features, scan3r.py:196-197) converted on load. */
int sga_gemm(int transA, int transB, int M, int N, int K, const void* A, long lda, int a_is_f64, const float* B,
             long ldb, float* C, long ldc, const float* bias, int accumulate, void* stream);
int sga_colsum(const float* X, long ld, int M, int N, float* out, int accumulate, void* stream);   /* bias grads */
/* C = A B^T (+ bias) for A [M,K], B [N,K] (Conv1d k=1 / Linear over point-major rows) with the BatchNorm batch statistics of C from the same
 * launch: sums[0..N) = column sums, sums[N..2N) = column sums of squares (fp64) -- sga_bn_stats without its pass over C.  Shapes the NT
 * kernel takes only (K % 4 == 0, 16-byte aligned rows); otherwise SGA_ERR_ARG and the caller uses sga_gemm + sga_bn_stats. */
int sga_gemm_bnstats(int M, int N, int K, const float* A, long lda, const float* B, long ldb, float* C, long ldc, const float* bias,
                     double* sums, void* stream);
int sga_cast_f64_f32(const double* in, float* out, size_t n, void* stream);                        /* .float(), sg_aligner.py:73-75 */
/* Which kernel a GEMM call takes -- the launcher's own decision, for tests that must know what they ran and for callers sizing a batch.  Host
 * only: with ncu > 0 (the CU count to plan for) no device is touched; ncu = 0 asks the current device.  a_aligned16 / b_aligned16: the operand
 * pointer is a multiple of 16 bytes.  accumulate / has_bias / has_resid / has_colstats (sga_gemm_bnstats) / act as the call would pass them.
 * route: one of sga_gemm_route; splits: workgroups along K (> 1: fp32 atomics into C, not run-to-run bit-stable); k_per_split: K rows of each.
 * SGA_GEMM_REFUSED (sga_gemm_bnstats on a shape the NT kernels do not take) still returns SGA_OK here; the launch returns SGA_ERR_ARG.
 * Row-chunk invariance: for K < 4096 the route of C = act(A B^T + bias) (+ resid) is a function of (N, K, alignment) and of M only through the
 * NT tile height (64 | 128 rows, equal bits), so a batch walked in chunks of rows gets the bits of the unchunked call; from K = 4096 on a call
 * of few rows is split over K (atomics) and that does not hold. */
enum sga_gemm_route {
    SGA_GEMM_EMPTY = 0,
    SGA_GEMM_TN_NARROW,
    SGA_GEMM_TN_SPLIT,
    SGA_GEMM_TN_BIG,
    SGA_GEMM_NN,
    SGA_GEMM_NT_128,
    SGA_GEMM_NT_64,
    SGA_GEMM_NT3_128,
    SGA_GEMM_NT3_64,
    SGA_GEMM_SMALL_F32,
    SGA_GEMM_SMALL_F64,
    SGA_GEMM_GENERIC_F32,
    SGA_GEMM_GENERIC_F64,
    SGA_GEMM_REFUSED
};
int sga_gemm_plan(int transA, int transB, int M, int N, int K, long lda, long ldb, long ldc, long ldr, int a_is_f64, int a_aligned16,
                  int b_aligned16, int has_bias, int accumulate, int act, int has_resid, int has_colstats, int ncu, int* route, int* splits,
                  int* k_per_split);

/* ---- modality fusion --------------------------------------------------------------------------------
 * replaces MultiModalFusion.forward, src/aligner/sg_aligner.py:30-35:
 *   joint[t, m*D:(m+1)*D] = softmax(weight)[m] * embs[m][t,:] / max(||embs[m][t,:]||, 1e-12)
 * embs: host array of M device pointers [T,D]; weight [M] (the [M,1] parameter); joint [T,M*D]. */
int sga_fusion_fwd(const float* const* embs, int M, const float* weight, float* joint, int T, int D, void* stream);
size_t sga_fusion_bwd_workspace_bytes(int M);
int sga_fusion_bwd(const float* const* embs, int M, const float* weight, const float* gjoint, float* const* gembs,
                   float* gweight, int T, int D, void* workspace, size_t workspace_bytes, void* stream);
/* The same for tables of DIFFERENT widths (the EVA baseline's 400 / 200 / 100 / 100 columns, src/aligner/eva.py:88-94): widths is a HOST
 * array of M column counts (each >= 1), embs[m] is [T, widths[m]], joint [T, sum widths] holds table m at column offset sum(widths[:m]).
 * Same arithmetic per table and row, same workspace (sga_fusion_bwd_workspace_bytes). */
int sga_fusion_var_fwd(const float* const* embs, int M, const int32_t* widths, const float* weight, float* joint, int T, void* stream);
int sga_fusion_var_bwd(const float* const* embs, int M, const int32_t* widths, const float* weight, const float* gjoint,
                       float* const* gembs, float* gweight, int T, void* workspace, size_t workspace_bytes, void* stream);

/* ---- GAT structure encoder --------------------------------------------------------------------------
 * replaces torch_geometric.nn.GATConv (2.2.0, un-vendored) as used by src/aligner/networks/gat.py:36-37,44,
 * for ALL graphs of a batch in one launch (sg_aligner.py:86-110 issues 2B sequential calls):
 * any GATConv(in, channels, heads) the reference's MultiGAT can stack (gat.py:35-37): heads >= 1 heads of 1 <= channels <= 256 channels each.
 * H [T, heads*channels] = x W^T head-major (as out / dO / dH), att_src / att_dst / bias / d_att_src / d_att_dst [heads*channels]; edges
 * [sumE,2] int64 graph-local (col 0 source, col 1 target); node_off/edge_off [G+1] int32 prefix sums; nmax = max nodes per graph (<= 256).
 * out[i] = sum_j softmax_j(leaky_relu(a_s[j]+a_d[i], 0.2)) H[j] + bias, self loops normalised as PyG does.
 * Limits the CALLER must respect (the Python wrapper checks the first two on the host once per batch): node ids are
 * graph-local in [0, nodes of that graph) -- an endpoint outside that range is DROPPED by the kernels, where PyG would raise;
 * duplicate edges count with their multiplicity (as PyG's scatter does) up to 255 copies of one (source, target) pair -- the
 * multiplicity matrix is 8-bit and saturates there; when that happens bit 0 of *status (device int32, caller-zeroed, may be NULL)
 * is set, and the Python wrapper turns it into an exception (deferred by at most one step, like the edge range check).
 * A graph with more than 256 nodes is rejected with SGA_ERR_ARG.  Both limits -- 256 nodes, 255 copies -- belong to THIS route, the dense
 * multiplicity matrix in LDS; the sparse route below (sga_gat_sp_*) has neither.
 * complete [G] uint8 (may be NULL): 1 = graph g lists every ordered pair i != j exactly once and nothing else -- what
 * preprocessing/scan3r/preprocess.py:176-182 writes for every scene (annotated relations + the supplemented 'none' pairs); its
 * multiplicities are all 1 and the kernels do not read its edges at all (16 B per edge: 2.13 GB at configs[2], eight times per step).
 * sga_gat_complete_flags fills the array from the edge lists themselves (order-independent: an N x N bitmap per graph), once per batch. */
int sga_gat_complete_flags(const int64_t* edges, const int32_t* node_off, const int32_t* edge_off, int G, uint8_t* flags, void* stream);
/* One workgroup per (graph, head); lanes span the channels in ceil(channels / 64) slots, the last one masked.  A head's features
 * [N, channels] (and, backward, their gradient's) are kept in LDS, row stride channels | 1, while they fit the 160 KiB of a CU beside the
 * multiplicity matrix: sga_gat_lds_nodes(channels, bwd) is the largest nmax for which they do (bwd != 0: the backward kernel's two copies);
 * above it the rows are read from global memory.  heads == 2 with channels == 128, the reference model's layers, launches kernels of its own
 * with those two numbers literal (the same algorithm; features in LDS up to 128 nodes, from global memory above).
 * heads < 1, channels < 1 or channels > 256 is SGA_ERR_ARG (sga_gat_lds_nodes: -1), before any device call. */
int sga_gat_attn_fwd_hc(const float* H, int heads, int channels, const float* att_src, const float* att_dst, const float* bias,
                        const int64_t* edges, const int32_t* node_off, const int32_t* edge_off, int G, int nmax,
                        float* out, int32_t* status, const uint8_t* complete, void* stream);
int sga_gat_attn_bwd_hc(const float* H, const float* dO, int heads, int channels, const float* att_src, const float* att_dst,
                        const int64_t* edges, const int32_t* node_off, const int32_t* edge_off, int G, int nmax, float* dH,
                        float* d_att_src, float* d_att_dst, const uint8_t* complete, void* stream);
/* The general kernels' residency boundary.  It has no head count: at channels == 128 it answers for every heads != 2 (215 forward, 135
 * backward); the launch at heads == 2, channels == 128 keeps features in LDS up to 128 nodes in both directions, whatever this returns. */
int sga_gat_lds_nodes(int channels, int bwd);
/* The SPARSE route: the same attention over a compressed edge list instead of a dense matrix in LDS -- graphs of ANY size, multiplicities of
 * 32 bits (no saturation, no status word), no atomics: every sum's order is fixed by the structure alone, so the outputs are bitwise
 * repeatable, a graph's out / dH rows are the same bits alone or inside a batch, and nothing depends on the order in which the edge list
 * names the edges.  Limits: 1 <= heads <= 65536, 1 <= channels <= 256 per head, T * heads below 2^31, cap = sum E + T at most 2^31 - 65.  The entry points above (the dense
 * route, at most 256 nodes per graph) are unchanged and remain the default of the Python layer.  The GCN runs over the same structure
 * through sga_gcn_sp_dinv / sga_gcn_sp_aggregate (below, with sga_gcn_aggregate).
 *
 * Structure, built on the device once per batch from the inputs of the dense route (T = node_off[G] nodes, E = edge_off[G] listed edges;
 * input self loops and endpoints outside [0, nodes of the graph) dropped, one self loop added per node, duplicates counted), over
 * batch-global node ids:
 *   row_ptr [T+1], src [cap], mult [cap]   target-major: the entries of target i are [row_ptr[i], row_ptr[i+1]), sources ascending
 *   col_ptr [T+1], tgt [cap], perm [cap]   its transpose: the entries of source j, targets ascending; perm = index of the target-major entry
 * U = row_ptr[T] = col_ptr[T] <= cap entries are used (U stays on the device); the slots behind them are zeroed.  The caller sorts:
 *   sga_gat_sp_keys      keys [cap] int64: target << 32 | source per listed edge and per self loop, INT64_MAX for a dropped edge
 *   (caller)             sorted_keys = sort(keys)
 *   sga_gat_sp_heads     head [cap] int32: 1 where a run of equal sorted keys begins
 *   (caller)             head_incl = inclusive prefix sum of head, int32
 *   sga_gat_sp_rows      row_ptr, src, mult and keys_t [cap] int64 (source << 32 | target per entry, INT64_MAX behind U);
 *                        workspace: sga_gat_sp_build_workspace_bytes(cap) bytes
 *   (caller)             sorted_keys_t, order_t = sort(keys_t) with the int64 slot each key came from
 *   sga_gat_sp_cols      col_ptr, tgt, perm
 * sga_gat_sp_capacity(T, E) = T + E, or -1 (message set) where that exceeds 2^31 - 65 (the kernels walk a segment in steps of 64 entries
 * with 32-bit positions); every call that takes cap refuses a larger one.
 * sga_gat_sp_fwd / sga_gat_sp_bwd: H / dO / out / dH [T, heads*channels] head-major, att_src / att_dst / bias / d_att_src / d_att_dst
 * [heads*channels], workspace of sga_gat_sp_workspace_bytes(T, cap, heads, channels, bwd) bytes (0: bad arguments, or nothing needed;
 * a smaller one is SGA_ERR_WORKSPACE).  T == 0 is a no-op; the backward still zeroes d_att_src / d_att_dst. */
int sga_gat_sp_capacity(int T, int E);
size_t sga_gat_sp_build_workspace_bytes(int cap);
size_t sga_gat_sp_workspace_bytes(int T, int cap, int heads, int channels, int bwd);
int sga_gat_sp_keys(const int64_t* edges, const int32_t* node_off, const int32_t* edge_off, int G, int T, int E, int64_t* keys, void* stream);
int sga_gat_sp_heads(const int64_t* sorted_keys, int cap, int32_t* head, void* stream);
int sga_gat_sp_rows(const int64_t* sorted_keys, const int32_t* head_incl, int cap, int T, int32_t* row_ptr, int32_t* src, int32_t* mult,
                    int64_t* keys_t, void* workspace, size_t ws_bytes, void* stream);
int sga_gat_sp_cols(const int64_t* sorted_keys_t, const int64_t* order_t, int cap, int T, int32_t* col_ptr, int32_t* tgt, int32_t* perm,
                    void* stream);
int sga_gat_sp_fwd(const float* H, int heads, int channels, const float* att_src, const float* att_dst, const float* bias,
                   const int32_t* row_ptr, const int32_t* src, const int32_t* mult, int T, float* out, void* workspace, size_t ws_bytes,
                   void* stream);
int sga_gat_sp_bwd(const float* H, const float* dO, int heads, int channels, const float* att_src, const float* att_dst,
                   const int32_t* row_ptr, const int32_t* src, const int32_t* mult, const int32_t* col_ptr, const int32_t* tgt,
                   const int32_t* perm, int T, int cap, float* dH, float* d_att_src, float* d_att_dst, void* workspace, size_t ws_bytes,
                   void* stream);
int sga_elu_fwd(const float* x, float* y, size_t n, void* stream);                    /* F.elu, gat.py:45-46 */
int sga_elu_bwd(const float* x, const float* gy, float* gx, size_t n, void* stream);

/* ---- GCN structure encoder (EVA baseline) -----------------------------------------------------------
 * replaces torch_geometric.nn.GCNConv(in, out, cached=False) as src/aligner/networks/gat.py:6-25 (MultiGCN) stacks it, for all graphs of a
 * batch in one launch.  H [T,C] = x W^T (any C >= 1), bias [C] or NULL; edges / node_off / edge_off / nmax / status as for the GAT kernels
 * above (graph-local ids, endpoints out of range dropped, at most 256 nodes per graph -- more is SGA_ERR_ARG --, 8-bit multiplicities
 * with bit 0 of *status set beyond 255 copies of one pair; both limits belong to this dense route, sga_gcn_sp_* below has neither).  Input self loops are removed, every node gets one self loop of weight 1,
 * deg_i = 1 + #{listed j -> i, j != i} (duplicates counted), dinv = deg^-1/2 correctly rounded to fp32, and
 *   transpose == 0:  out[i] = sum_{j -> i} dinv_i dinv_j H[j] + bias      (relu != 0: max(., 0) on top)
 *   transpose != 0:  out[j] = sum_{j -> i} dinv_i dinv_j H[i]             (the backward of the line above; bias NULL, relu 0)
 * duplicates as separate terms, the self loop included.  No floating-point atomics: the output is a pure function of the input.
 * out must not alias H.  sga_relu_bwd: gx = gy [y > 0] for y = relu(.). */
int sga_gcn_aggregate(const float* H, int C, const float* bias, const int64_t* edges, const int32_t* node_off, const int32_t* edge_off,
                      int G, int nmax, int transpose, int relu, float* out, int32_t* status, void* stream);
int sga_relu_bwd(const float* y, const float* gy, float* gx, size_t n, void* stream);
/* The SPARSE route of the GCN: the same arithmetic over the structure of sga_gat_sp_rows / sga_gat_sp_cols (batch-global node ids, ascending
 * neighbours, 32-bit multiplicities, one self loop per node) -- graphs of ANY size, any number of copies of a pair, no status word.
 *   sga_gcn_sp_dinv       dinv [T]: deg_i = the integer sum of mult over the target-major row of i (the self loop counts 1),
 *                         dinv_i = (float)(1.0 / sqrt((double)deg_i)), correctly rounded -- once per batch
 *   sga_gcn_sp_aggregate  one entry point for both directions, by the choice of arrays (ptr [T+1], nbr [cap], mult [cap], perm [cap] or NULL):
 *     forward    ptr = row_ptr, nbr = src, perm = NULL:   out[i] = sum_{entries e of row i} coef_e H[src_e] + bias   (relu != 0: max(., 0) on top)
 *     transpose  ptr = col_ptr, nbr = tgt, perm = perm:   out[j] = sum_{entries e of column j} coef_e H[tgt_e], the multiplicity read as
 *                mult[perm[e]]; bias must be NULL and relu 0 (anything else is SGA_ERR_ARG)
 *   coef_e = (float)mult_e * (dinv_out * dinv_nbr), two separately rounded multiplies.  Every output element is ONE fmaf chain from 0 in
 *   ascending neighbour order, the bias added after the chain, then the ReLU: the chain of sga_gcn_aggregate.  For a batch that route can
 *   take (at most 256 nodes per graph, no pair listed more than 255 times) both routes therefore return THE SAME BITS, in both directions.
 *   No floating-point atomics; a graph's rows are the same bits alone or inside a batch, whatever the order of the edge list.
 * H / out [T, C], any C >= 1 (C < 1: SGA_ERR_ARG "width %d < 1"); T < 0, cap < T or cap above 2^31 - 65 is SGA_ERR_ARG; a null pointer or out
 * aliasing H is refused before any device call; T == 0 is a no-op. */
int sga_gcn_sp_dinv(const int32_t* row_ptr, const int32_t* mult, int T, int cap, float* dinv, void* stream);
int sga_gcn_sp_aggregate(const float* H, int C, const float* bias, const int32_t* ptr, const int32_t* nbr, const int32_t* mult,
                         const int32_t* perm, const float* dinv, int T, int cap, int relu, float* out, void* stream);

/* ---- NCA loss (EVA baseline) --------------------------------------------------------------------------
 * replaces NCALoss.forward, src/aligner/losses.py:161-173, and its autograd, over row blocks of the score matrix s = Z1 Z2^T of the A
 * anchor pairs (Z from sga_loss_gather; the caller forms the block with sga_gemm).  S [h, lds >= A]: rows row0 .. row0 + h of s.
 *   S_ij = exp(alpha (s_ij - ep)) off the diagonal, 0 on it;  r_i = sum_j S_ij;  c_j = sum_i S_ij
 *   loss = mean_j log(1 + c_j) / alpha + mean_i log(1 + r_i) / alpha - beta mean_j log(1 + relu(s_jj))
 * sga_nca_block_sums: rsum[row0 .. row0 + h) (complete: a block holds whole rows), diag[row0 ..) = s_ii, and cpart [ceil(h / R), A]: the
 *   column sums over each group of R = sga_nca_row_group() consecutive rows of the block.  S is left as it is.
 * sga_nca_loss: cpart [ngroups, A] = the partials of ALL blocks stacked in block order -> csum [A], invr = 1 / (1 + r), invc = 1 / (1 + c)
 *   (fp32, [A]) and loss[0] (fp64).
 * sga_nca_coef: G [h, ldg >= A] := gout[0] * dloss/ds (G may be S itself, with ldg == lds: in place; a separate G leaves S untouched, so a
 *   kept block serves a second backward over the same graph),
 *     S_ij / A (invc_j + invr_i) off the diagonal,  -beta / A [s_jj > 0] / (1 + s_jj) on it,
 *   and GT [A, ldt >= h] := its transpose, columns h .. min(ldt, h rounded up to 4) zeroed (dZ1[block] = G Z2 and dZ2 += GT Z1[block]
 *   then need no transposed GEMM operand, and K may be taken as a multiple of 4).  Columns A .. ldg of G are left as they are.
 * Every sum is folded in a fixed order (fp32 within 256 columns of a row / 32 rows of a column, fp64 beyond): no floating-point atomics,
 * results bitwise repeatable. */
int sga_nca_row_group(void);
int sga_nca_block_sums(const float* S, long lds, int h, int A, int row0, float alpha, float ep, double* rsum, float* diag, double* cpart,
                       void* stream);
int sga_nca_loss(const double* rsum, const double* cpart, int ngroups, const float* diag, int A, float alpha, float beta, double* csum,
                 float* invr, float* invc, double* loss, void* stream);
int sga_nca_coef(const float* S, long lds, float* G, long ldg, float* GT, long ldt, int h, int A, int row0, float alpha, float beta, float ep,
                 const float* invr, const float* invc, const double* gout, void* stream);

/* ---- contrastive (ICL) / alignment (IAL) loss ---------------------------------------------------------
 * replace src/aligner/losses.py: calculate_prob_dist :5-15, ICLLoss.forward :43-58, IALLoss.forward :68-97.
 * Per table: Z [R,Dp] = packed, L2-normalised rows [e1i (A) | e2i (A) | e1j (J1) | e2j (J2)], Dp = D padded to 8. */
int sga_loss_gather(const float* E, int T, int D, const int32_t* idx, int R, float* Z, int Dp, float* nrm, void* stream);
int sga_loss_scatter(const float* dZ, const float* Z, const float* nrm, const int32_t* idx, int R, int D, int Dp,
                     float* dE, void* stream);                                  /* dE += J_normalize^T dZ (atomic) */
/* Scalar-accumulator buffers (sums8, sums, out, gs, gamma below) hold (1 + sga_loss_slots()) * n doubles: the first n
 * are the result, the rest per-wave partial slots (one shared set of addresses would serialise the fp64 atomics). */
int sga_loss_slots(void);
/* the four global sums of losses.py:10-11 at two temperatures: sums8[fam*2+temp], fam = s11,s12,s22,s21 */
int sga_loss_neg_sums(const float* Z, int Dp, int A, int J1, int J2, float tau0, float tau1, double* sums8, void* stream);
/* dZ += d(sums)/dZ weighted by gs8 = dL/d(sums8) (owner-stationary sweeps, atomic accumulate) */
int sga_loss_neg_grad(const float* Z, int Dp, int A, int J1, int J2, float tau0, float tau1, const double* gs8,
                      float* dZ, void* stream);
/* the same two for the anchor shard [a_lo, a_hi) this process owns: anchor-owner sweeps cover the shard only, negative-owner sweeps see
 * only the shard's anchors -- the outputs of a partition of [0, A) sum to the unsharded ones (one process per GPU all-reduces them) */
int sga_loss_neg_sums_shard(const float* Z, int Dp, int A, int J1, int J2, float tau0, float tau1, double* sums8, int a_lo, int a_hi,
                            void* stream);
int sga_loss_neg_grad_shard(const float* Z, int Dp, int A, int J1, int J2, float tau0, float tau1, const double* gs8,
                            float* dZ, int a_lo, int a_hi, void* stream);
/* anchors x anchors terms for NT tables (modalities..., joint): fwd: out = [NT icl sums | M iala | M ialb], M = NT-1;
 * bwd, given coef = dL/d(out): M1[k][j*A+i] = dL/dS_k[i,j] and gs[k][8] = dL/d(sums).
 * [a_lo, a_hi) (here and below): the anchor shard this process owns (0, A on one GPU).  Outputs are that shard's partial
 * contribution; the sum over a partition of [0, A) equals the unsharded result (one process per GPU all-reduces it).
 * Exact fp32 unless Zh is given: MFMA mode 'f16' (configs[4]: tables wider than 128 columns) takes fp16 INPUTS for the similarities of every
 * table k whose Zh[k] != NULL -- Zh[k] = the fp16 copy of Z[k]'s rows that sga_wide16_prepare writes (row pitch Dp[k] halfs); fp32 accumulate, the
 * epilogue unchanged.  Zh == NULL or Zh[k] == NULL: exact fp32 for that table.  1e-2 tolerance, like the mode's sweeps.
 * ws / ws_bytes (optional; sga_loss_anchor_f16_ws_bytes(NT, A, a_hi - a_lo) bytes; the caller passes it for WIDE tables): the 2 NT
 * similarity blocks of the shard (X1 X2^T and X2 X1^T, [A][a_hi - a_lo] fp32 each) are formed first -- tables with Zh[k] on the fp16 tile
 * core of the mode's sweeps (csrc/wide16.hip: 256 x 256 tiles, LDS-DMA), the others by the exact-fp32 NT GEMM (sga_gemm) -- and the kernels
 * run their epilogue only: same arithmetic, same results up to the fp32 summation order of the products.  ws == NULL: the one-kernel form. */
size_t sga_loss_anchor_f16_ws_bytes(int NT, int A, int ns);
int sga_loss_anchor_fwd_f16(const float* const* Z, const void* const* Zh, const int* Dp, int NT, int A, const double* sums,
                            float alpha, float tau_icl, float tau_ial, double* out, int a_lo, int a_hi, void* ws, size_t ws_bytes,
                            void* stream);
int sga_loss_anchor_bwd_f16(const float* const* Z, const void* const* Zh, const int* Dp, int NT, int A, const double* sums,
                            float alpha, float tau_icl, float tau_ial, const float* coef, float* const* M1,
                            double* gs, int a_lo, int a_hi, void* ws, size_t ws_bytes, void* stream);

/* dZ[a_lo:a_hi,:] += M1^T Z[A:2A,:] ; dZ[A:2A,:] += M1 Z[a_lo:a_hi,:]  (M1 [A, a_hi-a_lo] from sga_loss_anchor_bwd_f16; dZ zero-initialised) */
int sga_loss_stash_grad(const float* M1, const float* Z, int A, int Dp, float* dZ, int a_lo, int a_hi, void* stream);
/* fused variants for the normal pipeline, where the last table is the fusion of the M others: every joint
 * similarity is S_J = sum_m beta_m S_m (beta_m = w_m^2 / sum w^2, w = softmax(fusion.weight), sg_aligner.py:32-34
 * + losses.py:44,73), so the 300-d table is never multiplied.  Z[m] [R+32, 104] (Dp must be 104, 32 readable rows of
 * slack), D = the real embedding width (columns D..103 are zero padding; the K step that only covers padding is skipped),
 * beta [M] device.  sums/gs [(M+1)][8] with the joint in row M; gamma[m] += dL/dbeta_m through the negatives. */
int sga_loss_multi_sums(const float* const* Z, int M, int D, const float* beta, int A, int J1, int J2, float tau0, float tau1,
                        double* sums, int a_lo, int a_hi, void* stream);
int sga_loss_multi_grad(const float* const* Z, int M, int D, const float* beta, int A, int J1, int J2, float tau0, float tau1,
                        const double* gs, float* const* dZ, double* gamma, int a_lo, int a_hi, void* stream);
/* The same two fp32-MFMA sweeps with the gradient delivered in TWO parts (src/aligner/losses.py:43-58 through F.normalize's backward: a
 * table of nearly parallel rows -- meta_embedding_rel -- has an almost radial gradient, and the tangential part that survives the
 * normalisation's Jacobian must not be the rounding residue of a large radial sum).  sga_loss_centre_tables: packed table Z [R(+32), 104]
 * (R = 2A + J1 + J2) -> Zc [R(+32), 104] = (z - zbar | b = zbar.(z - zbar) + |zbar|^2/2 | 1 | 0 | 0), zbar = 0 unless |mean row|^2 >= 1/4
 * (same rule and same fixed-order column means as sga_loss_split3_tables); stat_ws: sga_loss_centre_bytes() bytes, receives the table's
 * statistics block.  The _centred sweeps take those tables (emb_dim <= 100): the owner side reads columns 100 / 101 swapped, so the MFMAs
 * still deliver S_ij = z_i . z_j; dZ[r, 0..100) += sum_j c_rj (z_j - zbar), dZ[r, 101] += sum_j c_rj.  The A x A stash products take Zc as
 * their B operand (sga_loss_stash_grad*: same two parts); sga_loss_scatter_tangent_stat projects G - rho (z_r - zbar). */
size_t sga_loss_centre_bytes(void);
int sga_loss_centre_tables(const float* Z, int A, int J1, int J2, float* Zc, void* stat_ws, void* stream);
int sga_loss_multi_sums_centred(const float* const* Zc, int M, const float* beta, int A, int J1, int J2, float tau0, float tau1,
                                double* sums, int a_lo, int a_hi, void* stream);
int sga_loss_multi_grad_centred(const float* const* Zc, int M, const float* beta, int A, int J1, int J2, float tau0, float tau1,
                                const double* gs, float* const* dZ, double* gamma, int a_lo, int a_hi, void* stream);
int sga_loss_scatter_tangent_stat(const float* dZ, const float* Z, const float* nrm, const int32_t* idx, int R, int D,
                                  const void* stat_ws, float* dE, void* stream);
/* fused anchors x anchors terms (M in {2,3,4}): same outputs as sga_loss_anchor_fwd_f16/bwd_f16 for tables (Z_1..Z_M, joint), with the
 * joint similarities derived in registers; bwd writes M1[m] = dL/dS_m + beta_m dL/dS_J (no joint stash) and gamma[m] += dL/dbeta_m.
 * bwd with out_terms != NULL ([(M+1) + 2M] doubles + slots, like `out` of the fwd call) ALSO returns the forward term values of the
 * anchor rows [a_lo, a_hi) from the same launch: a training step whose dL/d(terms) (`coef`) is known before the terms are -- the
 * standard loss head, losses.py:114-152 -- computes the A x A similarities once (ops.FusedContrastiveFn, one-pass mode). */
int sga_loss_anchor_multi_fwd(const float* const* Z, int M, const float* beta, int A, const double* sums, float alpha,
                              float tau_icl, float tau_ial, double* out, int a_lo, int a_hi, void* stream);
int sga_loss_anchor_multi_bwd(const float* const* Z, int M, const float* beta, int A, const double* sums, float alpha,
                              float tau_icl, float tau_ial, const float* coef, float* const* M1, double* gs, double* gamma,
                              int a_lo, int a_hi, double* out_terms, void* stream);
/* Symmetric form of the anchors x anchors backward (M in {2,3,4}; reference arithmetic losses.py:43-97, where term (i,j) and term (j,i)
 * are made of the same two similarities S[i,j], S[j,i]): rows [a_lo, a_hi) meet the columns [j_lo, j_hi) only; tiles at j >= mir also
 * produce the mirrored element (j, i) (stash M2, rows j - mir), tiles left of mir are visited in the ordered way and must lie in the
 * block's own square.  An UNSHARDED anchor set walked in blocks is (j_lo, j_hi, mir) = (a_lo, A, a_hi): block [a_lo, a_hi) meets the
 * columns j >= a_lo only and also evaluates the mirrored elements (j, i), j >= a_hi -- every unordered anchor pair once over the whole
 * walk instead of twice.  Other jobs serve ONE RANK of an anchor-sharded job (new design; the reference has no multi-GPU path:
 * src/engine/base_trainer.py:70,146-158 is dead).  a_lo % 32 == 0; a_hi % 32 == 0 or a_hi == A; j_lo, j_hi (or == A), mir (or >= j_hi)
 * multiples of 16.  M1[m]: [j_hi - j_lo, ns = a_hi - a_lo] floats, M1[m][(j-j_lo)*ns + (i-a_lo)] = dL/dS_m[i,j]; M2[m]: [j_hi - mir, ns],
 * M2[m][(j-mir)*ns + (i-a_lo)] = dL/dS_m[j,i] (M2 or M2[m] may be NULL when mir >= j_hi).  out_terms / gs / gamma: the block's share,
 * both elements of every pair it visits; summed over the blocks of a walk they equal sga_loss_anchor_multi_bwd's over the same rows.
 * sga_loss_stash_grad_symx applies one table's two stashes: dX1[R] += M1^T X2[j_lo:j_hi], dX2[j_lo:j_hi] += M1 X1[R],
 * dX1[mir:j_hi] += M2 X2[R], dX2[R] += M2^T X1[mir:j_hi]  (R = [a_lo, a_hi)). */
int sga_loss_anchor_multi_bwd_symx(const float* const* Z, int M, const float* beta, int A, const double* sums, float alpha,
                                   float tau_icl, float tau_ial, const float* coef, float* const* M1, float* const* M2,
                                   double* gs, double* gamma, int a_lo, int a_hi, int j_lo, int j_hi, int mir, double* out_terms, void* stream);
int sga_loss_stash_grad_symx(const float* M1, const float* M2, const float* Z, int A, int Dp, float* dZ, int a_lo, int a_hi,
                             int j_lo, int j_hi, int mir, void* stream);

/* *poison = NaN if any row norm is below F.normalize's eps (the identity above would not hold): fail loudly */
int sga_loss_check_norms(const float* nrm, int n, float* poison, void* stream);

/* ---- the two fused sweeps with every fp32 operand split EXACTLY into three bf16 terms (ops.set_mfma_mode('bf16x6'); sweep3.hip) ------
 * replaces src/aligner/losses.py:5-15 (calculate_prob_dist's anchors x negatives products) and its autograd, like sga_loss_multi_sums /
 * sga_loss_multi_grad, in fp32 arithmetic on the bf16 matrix pipe: x = h + m + l (8 + 8 + 8 significand bits, fp32's exponent range: every
 * fp32 value exactly), a product = the six partial products down to 2^-16 relative on v_mfma_f32_16x16x32_bf16 into one fp32 accumulator
 * (the dropped three are <= 2^-23 of the product), i.e. 6/16 of the fp32 MFMA's matrix time at fp32's own accuracy ("fp32 MFMA
 * or split-bf16 x3").  M = 2, 3 or 4 tables, emb_dim <= 100 (columns 100, 101 of the planes carry the row centring's bookkeeping); M = 4's
 * gradient runs as two launches, each forming all four similarities and the owner gradients of two tables (the accumulators of four
 * tables do not fit a wave's registers).
 * sga_loss_split3_tables: packed fp32 table Z [R(+32), 104] -> Zb, 32-row blocks of bf16 h / m / l planes in MFMA operand order + one
 * packed K-tail image (sga_loss_split3_bytes bytes; segments X1 | X2 | N1 | N2 each padded to whole blocks; column means summed in a
 * fixed order: the planes are bitwise reproducible).  The other arguments and every output: as sga_loss_multi_sums / sga_loss_multi_grad,
 * except that the gradient arrives in TWO parts: dZ[r, 0..100) += sum_j c_rj (z_j - zbar) and dZ[r, 101] += sum_j c_rj (zbar = 0 unless the
 * table's rows are nearly parallel, |mean row|^2 >= 1/4).  Zc (optional) receives the anchor rows as fp32 [2A, 104] = z - zbar with column
 * 101 = 1: the B operand that makes sga_loss_stash_grad* deliver the A x A part in the same two-part form.
 * sga_loss_scatter_tangent = sga_loss_scatter (the autograd of F.normalize + the row gather, losses.py:44-48) for that form: it projects
 * G - rho (z_r - zbar) instead of the summed gradient -- identical in exact arithmetic (P_r z_r = 0), and free of the cancellation that
 * costs a table of nearly parallel rows 3e-4 of its gradient when the radial part is formed in fp32 first. */
size_t sga_loss_split3_bytes(int A, int J1, int J2);
int sga_loss_split3_tables(const float* Z, int A, int J1, int J2, void* Zb, float* Zc, void* stream);
/* lite != 0 (forward sums only): similarities from the h and m planes alone (products h h + h m + m h, exact K tail; 11 instead of 20 MFMAs
 * and no l-plane traffic) -- every similarity with an unbiased ~2^-16 rounding; for global sums of >= 2^24 terms each (the caller's call) they move by
 * < 1e-7 relative.  lite == 0: all six products. */
int sga_loss_multi_sums_bf16x6(const void* const* Zb, int M, const float* beta, int A, int J1, int J2, float tau0, float tau1,
                               double* sums, int a_lo, int a_hi, int lite, void* stream);
int sga_loss_multi_grad_bf16x6(const void* const* Zb, int M, const float* beta, int A, int J1, int J2, float tau0, float tau1,
                               const double* gs, float* const* dZ, double* gamma, int a_lo, int a_hi, void* stream);
int sga_loss_scatter_tangent(const float* dZ, const float* Z, const float* nrm, const int32_t* idx, int A, int J1, int J2, int D,
                             const void* Zb, float* dE, void* stream);
/* The four stash products of sga_loss_stash_grad_symx (same M1 / M2 / block arguments; a_lo = 0, a_hi .. with j_lo = 0, j_hi = mir = A it is
 * sga_loss_stash_grad) on the three exact bf16 planes Zb of sga_loss_split3_tables: fp32 coefficients split in registers, six bf16 MFMAs per
 * product, fp32 accumulation; dZ [2A.., 104] receives the two-part form (columns 0..99 and 101) that sga_loss_scatter_tangent projects. */
int sga_loss_stash_grad_symx_bf16x6(const float* M1, const float* M2, const void* Zb, int A, int J1, int J2, float* dZ,
                                    int a_lo, int a_hi, int j_lo, int j_hi, int mir, void* stream);
/* How that entry point cuts a job into workgroups on a device of `cus` compute units; launches nothing and needs no device.
 * plan[25] = {workgroups, then per product (up to four, unused ones zero) {owner rows, first 32-row tile, end tile, nsplit, first workgroup,
 * transposed}}: workgroup blk0 + s * nob + ob of a product (nob = ceil(owner rows / 128)) takes owner rows 128 ob .. and the tiles
 * [t0 + s per, min(t1, t0 + (s + 1) per)), per = ceil((t1 - t0) / nsplit).
 * sga_loss_stash_unit_tiles: the length in tiles that a work unit aims at (0: the library's default; every product still gets ~4
 * workgroups per CU); -n: units of exactly n tiles whatever the fill (small jobs in tests).  Returns the value before.  Process-wide;
 * for tests and timing. */
int sga_loss_stash_plan(int A, int a_lo, int a_hi, int j_lo, int j_hi, int mir, int cus, int32_t* plan);
int sga_loss_stash_unit_tiles(int tiles);
/* sga_loss_anchor_multi_bwd_symx with the similarities formed from the three-plane images Zb[m] of sga_loss_split3_tables (same A, J1, J2;
 * their anchor segments X1 | X2) on the bf16 matrix pipe: the sweeps' six partial products in one fp32 accumulator, then the fp32 kernel's
 * own epilogue.  M = 2 or 3.  Same outputs: stash layouts, gs / gamma / out_terms slots and their fold.  a_lo, j_lo, mir: multiples of 32
 * (or mir >= j_hi: no mirrored elements, M2 may be NULL); a_hi, j_hi: multiples of 32 or == A.  The ordered walk of a block is
 * (j_lo, j_hi, mir) = (0, A, A), M2 == NULL; only then may out_terms be NULL (no term values). */
int sga_loss_anchor_multi_bwd_symx_bf16x6(const void* const* Zb, int M, const float* beta, int A, int J1, int J2, const double* sums,
                                          float alpha, float tau_icl, float tau_ial, const float* coef, float* const* M1, float* const* M2,
                                          double* gs, double* gamma, int a_lo, int a_hi, int j_lo, int j_hi, int mir, double* out_terms,
                                          void* stream);
/* How an A x A backward job (rows [a_lo, a_hi) x columns [j_lo, j_hi)) is cut into workgroups on `slots` workgroup slots (on a device: CUs x
 * resident workgroups of the kernel); launches nothing and needs no device.  planes != 0: the three-plane entry point above, else
 * sga_loss_anchor_multi_bwd / _symx.  plan[8] = {R rows of a row block, H 16-column halves a workgroup walks side by side per step, nib row
 * blocks, nib1, n1, n2, workgroups, steps of a row block}: workgroup w < nib1 * n1 is (row block w / n1, split w % n1 of n = n1), the
 * others follow from row block nib1 on with n = n2; split s of n walks the steps s, s + n, ... of its row block, step t being the halves
 * j_lo / 16 + H t .. + H - 1.  The first run fills whole rounds of workgroups, the second, cut finer, the last one. */
int sga_loss_anchor_plan(int planes, int M, int A, int a_lo, int a_hi, int j_lo, int j_hi, int slots, int32_t* plan);

/* ---- loss_group = b: the same loss on G independent groups of b consecutive pairs ------------------------
 * replaces the reference trainer feeding b pairs per iteration (configs/scan3r/scan3r_ground_truth.yaml:27,
 * src/engine/epoch_based_trainer.py:91-93 -> src/aligner/losses.py:114-152) for all B/b groups of a device batch at once:
 * out[g] / gradients equal OverallLoss's raw terms evaluated on group g alone (its anchors against ITS negatives only).
 * Z[m] [R, 104] packed normalised tables (sga_loss_gather, Dp = 104), rows X1 | X2 | N1 | N2; beta [M] as in the fused
 * global path (NULL for M == 1: ICL only).  groups [G][8] int32 = {first anchor, #anchors, first N1 row, #N1, first N2
 * row, #N2, 0, 0} (contiguous ranges inside [0,A) / [0,J1) / [0,J2)); s_off [G+1] int64 float offsets of the groups'
 * similarity blocks [2 na, na+nj1+nj2] inside one table's slab of S [M][s_total].  sums [G][NT][8], out [G][NT+2M]
 * (NT = M+1, or 1 and no IAL columns when M == 1).  bwd: coef [G][NT+2M] = dL/d(out); S (as left by fwd) is overwritten
 * with dL/dS; dZ[m] += this batch's gradient (every packed row has one writer); gamma [G][M] = dL/dbeta per group.
 * use_valu: 1 = the VALU forms of the similarity / gradient kernels (kept for cross-checks), 0 = MFMA (what the product passes). */
int sga_group_loss_fwd(const float* const* Z, int M, const float* beta, int A, int J1, const int32_t* groups, int G,
                       const int64_t* s_off, int64_t s_total, float alpha, float tau_icl, float tau_ial, float* S,
                       double* sums, double* out, int use_valu, void* stream);
int sga_group_loss_bwd(const float* const* Z, int M, const float* beta, int A, int J1, const int32_t* groups, int G,
                       const int64_t* s_off, int64_t s_total, float alpha, float tau_icl, float tau_ial, float* S,
                       const double* sums, const float* coef, float* const* dZ, double* gamma, int use_valu, void* stream);

/* ---- per-pair similarity + ranking --------------------------------------------------------------------
 * replaces eval_step's emb/||emb||, sim = 1 - emb emb^T, argsort (src/inference/sgaligner/inference_align_reg.py:
 * 125-128) fused with the rank look-ups of utils/alignment.py:3-25,27-41,59-70.  The per-pair E E^T blocks run on the
 * matrix cores (exact fp32 MFMA; f16 != 0: fp16 inputs / fp32 accumulate on the normalised rows -- BASELINE.json
 * configs[4]).  pair_off [B+1] object offsets of the pairs; blk_pair / blk_row [n_blocks]: the (pair, 64-row block) of every
 * workgroup -- list exactly the blocks that contain a query object (any order; the caller knows q_idx), so that no workgroup is
 * launched for nothing and the work spreads over all XCDs.  For query object q_idx[q] (each object at most once): rank[q] = 1-based
 * rank of q_tgt[q] among its pair's other objects (q_tgt NULL or out of the pair: -1); topk_*[q,:K] its K nearest
 * others (pair-local index, distance), ascending, ties by index.  K <= 8, <= 512 objects per pair. */
size_t sga_simrank_workspace_bytes(int T);
size_t sga_simrank_workspace_bytes_f16(int T, int D);   /* workspace for f16 != 0: + the normalised fp16 table when D > 416 */
int sga_simrank(const float* E, int T, int D, const int32_t* pair_off, const int32_t* blk_pair, const int32_t* blk_row, int n_blocks, int B,
                int max_pair_objects, const int32_t* q_idx, const int32_t* q_tgt, int Q, int K, int32_t* rank,
                int32_t* topk_idx, float* topk_sim, int f16, void* workspace, size_t workspace_bytes, void* stream);
/* per pair b (queries pair_q_off[b]..pair_q_off[b+1], in sga_simrank's order): out[b][0..4] = Hits@1..5 counts,
 * [5] = #queries, [6] = sum 1/rank, [7..9] = SGAR for modes '2', '50', '100' (utils/alignment.py:13-25,3-11,27-57);
 * topk_* with leading dimension K >= 1 (column 0 = the top-1 prediction).  out [B][12] floats. */
int sga_pair_metrics(const int32_t* rank, const int32_t* topk_idx, const float* topk_sim, int K, const int32_t* q_tgt,
                     const int32_t* pair_off, const int32_t* pair_q_off, int B, float* out, void* stream);

/* ---- Point-Cloud-Transformer object encoder, inference path ('pct' module) ---------
 * sga_gemm_ex: C = act(op(A) op(B) + bias) (+ resid), act 0 none / 1 ReLU / 2 LeakyReLU(0.2): the conv1d(k=1) +
 *   eval-mode BatchNorm (folded into weight and bias by the caller) + activation (+ SA residual) layers of
 *   src/aligner/networks/pct.py:115-124 (Embedding), :223-229 (SA tail), :289-293 (linear), :311-315 (head).
 * sga_pct_attention: SA.forward's attention (pct.py:211-222) for T objects of N points each, flash style:
 *   Q [T*N,32] (= q_conv(x) = k_conv(x): shared weight, pct.py:199), V [T*N,128] (= v_conv(x) + bias) ->
 *   Xs[j,:] = sum_i softmax_row_i(Q Q^T / sqrt(32))[i,j] V[i,:].  stats: 2*T*N floats of workspace.
 * sga_segment_max: G[t,c] = max over the N points of object t (pct.py:308), argmax (nullable) = the winning point;
 * sga_segment_max_bwd: its backward, dY[t*N + argmax[t,c], c] = dG[t,c], zero elsewhere. */
int sga_gemm_ex(int transA, int transB, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
                float* C, long ldc, const float* bias, int act, const float* resid, long ldr, void* stream);
int sga_pct_attention(const float* Q, long ldq, const float* V, long ldv, int T, int N, float* stats, float* Xs,
                      long ldx, void* stream);
/* backward of sga_pct_attention (autograd of pct.py:211-222): stats as left by the forward, work = T*N floats */
int sga_pct_attention_bwd(const float* Q, long ldq, const float* V, long ldv, const float* dXs, long ldd, int T, int N,
                          const float* stats, float* work, float* dQ, long ldo, float* dV, long ldw, void* stream);
/* Offset attention, OA.forward (pct.py:261-269), for T objects of N >= 1 points each (T = 0: nothing is done).  Against sga_pct_attention:
 * no 1/sqrt(32), and the row softmax is L1-normalised over its COLUMNS before it is applied:
 *   E = Q Q^T,  P[i,j] = exp(E[i,j] - m_i) / l_i,  d_j = 1e-9f + sum_i P[i,j],  Xr[j,:] = (sum_i P[i,j] V[i,:]) / d_j.
 * The same kernels as sga_pct_attention (csrc/pct.hip, templated on the variant): the row-statistics pass, then the apply pass, whose lane
 * owns output row j, also adds up its column of P in-lane and divides at the end.  Exact fp32 MFMA, no atomics: an object's outputs have
 * the same bits alone and in a batch.
 *   Q [T*N,32], V [T*N,128], Xr [T*N,128] with their row strides (Q and V rows 16-byte aligned);  stats: 3*T*N floats, m | l | d;
 *   X (nullable) [T*N,128]: the layer's input;  Diff (nullable, needs X): X - Xr, the operand of trans_conv (pct.py:270).
 * sga_pct_offset_attention_bwd, with G = gsign * (the caller's gradient) = dL/dXr (gsign = -1 for a caller that holds dL/dDiff):
 *   Gh[j] = G[j] / d_j,  kappa_j = -<G[j], Xr[j]> / d_j,  dV[i] = sum_j P[i,j] Gh[j],  dP[i,j] = <V[i], Gh[j]> + kappa_j,
 *   delta_i = <V[i], dV[i]> + sum_j P[i,j] kappa_j,  dE = P (dP - delta_i),  dQ[i] = sum_j (dE[i,j] + dE[j,i]) Q[j].
 *   stats as left by the forward;  work: exactly T*N*130 floats, 16-byte aligned (Gh [T*N,128] | kappa [T*N] | delta [T*N]).
 * sga_segment_mean: G[t,c] = mean over the N points of object t (SPCT's x_mean, pct.py:349) in a fixed order -- four row walkers
 *   (rows n, n+4, ...) folded 0,1,2,3 -- and sga_segment_mean_bwd: dY[t*N + n, c] = dG[t,c] / N. */
int sga_pct_offset_attention(const float* Q, long ldq, const float* V, long ldv, const float* X, long ldxi, int T, int N, float* stats,
                             float* Xr, long ldx, float* Diff, long ldf, void* stream);
int sga_pct_offset_attention_bwd(const float* Q, long ldq, const float* V, long ldv, const float* Xr, long ldx, const float* G, long ldg,
                                 float gsign, int T, int N, const float* stats, float* work, float* dQ, long ldo, float* dV, long ldw,
                                 void* stream);
int sga_segment_mean(const float* Y, long ldy, int T, int N, int C, float* G, void* stream);
int sga_segment_mean_bwd(const float* dG, int T, int N, int C, float* dY, long ldd, void* stream);
int sga_segment_max(const float* Y, long ldy, int T, int N, int C, float* G, int32_t* argmax, void* stream);
int sga_segment_max_bwd(const float* dG, const int32_t* argmax, int T, int N, int C, float* dY, long ldd, void* stream);
/* Backward of conv(512->1024, no bias) + BatchNorm + LeakyReLU(slope) + max over an object's points (pct.py:282-286,306-308) without the
 * [T*N, 1024] gradient tensors: only arg-max rows carry dL/dz and the batch-statistic terms are affine in y = cat W^T, so
 *   dW = a (x) colsum(cat) + diag(b) W (cat^T cat) + sparse,   dcat = 1 (x) a^T W + cat (W^T diag(b) W) + sparse    (pct_ops.LinearBNActMaxFn).
 * head_prep: dG/G [T,C] (gradient / value of the pooled output), fin = [scale|shift|mean|rstd] of sga_bn_finalize, R = T*N rows ->
 *   coef [T,C] = scale * dL/dz at the arg-max rows, ab [4C] = a | b | dgamma | dbeta.   head_dw: WG = W (cat^T cat) [C,K], cs = colsum(cat) [K]
 *   -> dW [C,K], Wb = diag(b) W [C,K], a0 += a^T W [K] (caller-zeroed).   head_scatter: dcat[t N + amax[t,c], :] += coef[t,c] W[c,:]. */
int sga_pct_head_prep(const float* dG, const float* G, const float* gamma, const float* beta, const float* fin, int T, int C, long R,
                      int training, float slope, float* coef, float* ab, void* stream);
int sga_pct_head_dw(const float* WG, const float* W, const float* ab, const float* cs, const float* coef, const int32_t* amax,
                    const float* cat, long ldc, int T, int N, int C, int K, float* dW, float* Wb, float* a0, void* stream);
int sga_pct_head_scatter(const float* coef, const int32_t* amax, const float* W, int T, int N, int C, int K, float* dcat, long ldd,
                         void* stream);
/* G[t,c] = max_n LeakyReLU_slope(scale[c] Y[t N + n, c] + shift[c]) with its first arg-max row: BatchNorm-apply + activation folded into
 * the point max of that stage (Y read once, never rewritten); same numbers as sga_bn_apply + sga_segment_max. */
int sga_segment_max_affine(const float* Y, long ldy, int T, int N, int C, const float* scale, const float* shift, float slope, float* G,
                           int32_t* argmax, void* stream);

/* BatchNorm1d over point-major activations [R, C] fused with the following activation (0 none, 1 ReLU, 2 LeakyReLU 0.2)
 * and residual: the train-mode layers of pct.py:122-123, :226-229, :289-293, :311-315.  sums: 2*C doubles.
 *   sga_bn_stats:     sums = [sum_r x | sum_r x^2]
 *   sga_bn_apply:     Y = act(X * scale + shift) (+ resid)       (scale = gamma * rstd, shift = beta - mean * scale)
 *   sga_bn_bwd_stats: sums = [sum_r g | sum_r g * xhat],  g = dY * act'(X * scale + shift)    (= dbeta | dgamma)
 *   sga_bn_bwd_apply: dX = scale * (g - mean_g - xhat * mean_gx)   (mean_g / mean_gx NULL: eval-mode BN, dX = scale * g) */
int sga_bn_stats(const float* X, long ldx, int R, int C, double* sums, void* stream);
/* per-channel arithmetic between the passes as one launch each: out = [scale | shift | mean | rstd] (4C floats), running statistics and
 * num_batches_tracked (int64, may be NULL) updated like nn.BatchNorm1d when training != 0 (eval: the running statistics, sums unused);
 * backward: out = [dbeta | dgamma | mean_g | mean_gx] from the sums of sga_bn_bwd_stats. */
int sga_bn_finalize(const double* sums, int R, int C, const float* gamma, const float* beta, float* running_mean, float* running_var,
                    long long* num_batches_tracked, float momentum, float eps, int training, float* out, void* stream);
int sga_bn_bwd_finalize(const double* sums, int R, int C, float* out, void* stream);
int sga_bn_apply(const float* X, long ldx, int R, int C, const float* scale, const float* shift, int act,
                 const float* resid, long ldr, float* Y, long ldy, void* stream);
int sga_bn_bwd_stats(const float* X, long ldx, const float* dY, long ldd, int R, int C, const float* scale,
                     const float* shift, const float* mean, const float* rstd, int act, double* sums, void* stream);
int sga_bn_bwd_apply(const float* X, long ldx, const float* dY, long ldd, int R, int C, const float* scale,
                     const float* shift, const float* mean, const float* rstd, const float* mean_g,
                     const float* mean_gx, int act, float* dX, long ldo, void* stream);

/* ---- per-object farthest-point sampling (the step in front of the path) -----------------
 * replaces utils/point_cloud.py:61-89 pcl_farthest_sample as called by preprocessing/scan3r/preprocess.py:96-98.
 * pts [sum N,3] f32 packed per object, offsets [n_obj+1]; start[obj] = the first sample (the reference draws it with
 * np.random.randint, :77 -- the caller owns the RNG); out_idx [n_obj, npoint] object-local indices, bit-identical to
 * the reference's sequence for the same start (fp32, same summation order, first arg-max).  Every object needs
 * N >= npoint (the reference's N < npoint branch is a random draw with replacement and stays on the host).
 * work_small / work_mid / work_large: device lists of object ids with N <= 2048, <= 8192, > 8192 points (register-
 * resident vs global-walk kernels); scratch: sga_fps_scratch_floats(total points) floats, only read when n_large > 0. */
size_t sga_fps_scratch_floats(int total_points);
int sga_fps(const float* pts, const int32_t* offsets, int n_obj, const int32_t* start, int npoint,
            const int32_t* work_small, int n_small, const int32_t* work_mid, int n_mid,
            const int32_t* work_large, int n_large, int32_t* out_idx, float* scratch, void* stream);

/* ---- convex-hull candidate filter (the other half of the step in front of the path) ----------
 * serves preprocessing/scan3r/preprocess.py:93-96 (hull = ConvexHull(obj_pcl); barycentre = mean of the hull vertices):
 * keep[i] = 0 for points that are provably interior to their object's hull (strictly inside the convex hull of the object's 26
 * directional support points, by 1e-5 of its extent), 1 otherwise -- the hull of the kept points IS the object's hull, so the
 * host's Qhull call sees a few per cent of the points and returns the same vertices.  pts [sum N,3] f32 packed per object,
 * offsets [n_obj+1]; n_planes [n_obj] (nullable): facets of the filter polytope, 0 = object kept whole (degenerate). */
int sga_hull_candidates(const float* pts, const int32_t* offsets, int n_obj, unsigned char* keep, int32_t* n_planes, void* stream);
/* The hull VERTICES of every object's candidates on the device: fp64 gift wrapping with a certificate (closed surface, Euler's
 * relation, every other point behind every facet by > 1e-9 of the object's scale).  pts [sum n, 3] f64 packed per object (the survivors
 * of sga_hull_candidates, in the object's own values), offsets [n_obj+1].  status[o] == 0: is_vertex[offsets[o] ..] flags exactly the
 * vertices scipy.spatial.ConvexHull (Qhull) reports (one copy of bitwise-duplicate points); != 0 (fewer than 4 or more than
 * sga_hull_max_candidates() points, coplanar / near-degenerate facets, any failed check): is_vertex is untouched and the caller
 * must run Qhull on that object (utils/point_cloud.py does).  preprocessing/scan3r/preprocess.py:93-96. */
int sga_hull_max_candidates(void);
int sga_hull_vertices(const double* pts, const int32_t* offsets, int n_obj, unsigned char* is_vertex, int32_t* status, void* stream);

/* ---- batched exact nearest-neighbour search, fp64 (the point-cloud geometry either side of the path) ----------
 * replaces utils/point_cloud.py:136-147 get_nearest_neighbor (cKDTree(s).query(q, k=1)), the radius search of utils/point_cloud.py:91-103
 * compute_pcl_overlap (preprocessing/scan3r/subgenscan3r.py:107-118: every pair of subscans of every scan) and the per-vertex KD-tree loop
 * of utils/registration.py:107-129 nn_correspondence.  Brute force, so exact.
 * pts [total_points, 3] f64, clouds packed back to back; offsets [n_clouds + 1]; pairs [n_pairs, 2] = (query cloud, support cloud);
 * out_offsets [n_pairs]: where job p's nq results start in out_dist / out_idx [total_queries] (jobs must not overlap).  These three are
 * DEVICE int32 arrays; offsets_host / pairs_host (nullable) are host copies of offsets / pairs that, when given, are validated before
 * anything is launched.  max_queries / max_support: the largest query / support cloud of any job (they size the grid; a job larger than
 * stated is left partly unwritten, never read or written out of bounds -- the kernels re-check every id and offset they read).
 * Arithmetic: d2 = (dx*dx + dy*dy) + dz*dz, dx = q.x - s.x ..., each operation rounded on its own (no FMA); out_dist = d2 when squared != 0,
 * else the correctly rounded sqrt(d2): bit-identical to cKDTree's distances.  out_idx: the support-cloud-local index of the nearest
 * point; among exactly equal minima the LOWEST index (numpy.argmin's rule; cKDTree's choice is arbitrary).  Empty support: +inf, -1.
 * A NaN distance never wins.  chunk: support points per workgroup pass.  Jobs with ns <= chunk are finished in one pass; larger ones go
 * chunk by chunk into `workspace` (sga_nn_workspace_bytes(): 12 bytes x ceil(max_support / chunk) x total_queries, 0 when nothing is
 * split) and a second kernel folds the chunks in ascending order.  No atomics: the output is a pure function of the input. */
size_t sga_nn_workspace_bytes(int total_queries, int max_support, int chunk);
int sga_nn_search(const double* pts, const int32_t* offsets, int n_clouds, int total_points, const int32_t* pairs, int n_pairs,
                  const int32_t* out_offsets, int total_queries, int max_queries, int max_support, int chunk,
                  const int32_t* offsets_host, const int32_t* pairs_host, int squared, double* out_dist, int32_t* out_idx,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- batched exact-fp32 nearest-neighbour search in feature space, fp32 matrix cores -------------------------------------------
 * the matching step of utils/open3d.py:137-170 registration_with_ransac_from_feats (every source descriptor to its nearest reference
 * descriptor) and of src/engine/registration_evaluator.py:92-127: a GEMM with an arg-min epilogue on v_mfma_f32_32x32x2_f32.
 * feats [total_rows, C] f32 row-major, feature sets packed back to back, C >= 1 and C % 4 == 0, base 16-byte aligned (pad other widths
 * with zero columns: they change nothing); offsets [n_sets + 1]; pairs [n_pairs, 2] = (query set, support set); out_offsets [n_pairs]:
 * where job p's nq results start in out_idx / out_d2 [total_queries] (jobs must not overlap); tiles [n_tiles, 3] = (job, query tile of
 * 128 rows, chunk): the grid, one workgroup per entry -- every (query tile, chunk) a job has, nothing for those it has not; the first
 * n_query_tiles entries are the chunk-0 entries (one per query tile of every job), which also drive the closing kernel.  These are
 * DEVICE int32 arrays; offsets_host / pairs_host / tiles_host (nullable) are host copies that, when given, are validated before anything
 * is launched.  max_queries / max_support: the largest query / support set of any job (they size the partial workspace; the kernels
 * re-check every id and offset they read -- a bad one makes a workgroup do nothing, never read or write out of bounds).
 * Arithmetic: score s_j = n_j - 2 * dot_j in fp32, n_j = |b_j|^2 as an ascending fmaf chain, dot_j the MFMA's k-ordered fmaf chain (the
 * fixed k order is documented at the top of csrc/featnn.hip): a pure function of the two rows.  out_idx: the support-set-local arg-min
 * of s_j, the LOWEST index among exactly equal scores; a NaN score never wins; an empty support (or no score below +inf) gives -1.
 * out_d2 (f64) is recomputed for the chosen row alone: sum_k (double(a_k) - double(b_k))^2, k ascending, each operation rounded on its
 * own; +inf with -1.  chunk: support rows per workgroup pass.  Jobs with ns <= chunk are finished in one pass; larger ones write
 * per-chunk (score, idx) partials that are folded in ascending chunk order.  workspace (sga_featnn_workspace_bytes()): 4 bytes x
 * total_rows for the norms, rounded up to 8, plus 8 bytes x ceil(max_support / chunk) x total_queries when anything is split.  No
 * atomics: the output is a pure function of the input. */
size_t sga_featnn_workspace_bytes(int total_rows, int total_queries, int max_support, int chunk);
int sga_featnn_search(const float* feats, int C, const int32_t* offsets, int n_sets, int total_rows, const int32_t* pairs, int n_pairs,
                      const int32_t* out_offsets, const int32_t* tiles, int n_tiles, int n_query_tiles, int total_queries, int max_queries,
                      int max_support, int chunk, const int32_t* offsets_host, const int32_t* pairs_host, const int32_t* tiles_host,
                      int32_t* out_idx, double* out_d2, void* workspace, size_t workspace_bytes, void* stream);

/* ---- FPFH descriptors: exact neighbour lists, normals, SPFH census, FPFH weighting (fp64; csrc/fpfh.hip) ----------------------------
 * the descriptor side of utils/open3d.py:61-66 (estimate_normals), :78-86 and :137-170: points -> neighbour lists -> normals -> SPFH -> FPFH,
 * whose fp32 output feeds sga_featnn_search.  Open3D is not a dependency and equality with its output is not tested: the text below is
 * the definition (tests/fpfh_ref.py restates it in numpy).  All four entries take clouds packed back to back: pts [total_points, 3] f64,
 * offsets [n_clouds + 1] DEVICE int32; offsets_host (nullable) is a host copy that, when given, is validated before anything is launched.
 * The kernels re-check every offset, count and index they read: a bad one makes them do nothing (or skip that neighbour), never read or
 * write out of bounds.  Neighbours are always taken from the point's own cloud; indices are cloud-local.  1 <= max_nn <= 128 (the lists'
 * row width in every entry).  No floating-point atomics: every output is a pure function of the input.  Stream-ordered, no workspace.
 *
 * sga_knn_lists: for point i the first max_nn entries of { j : d2(i, j) <= r2 } sorted ascending by (d2, j), j over the whole cloud (the
 * point itself included, d2 = 0).  d2 = (dx*dx + dy*dy) + dz*dz, each operation rounded on its own: sga_nn_search's arithmetic, bit for
 * bit.  r2 = +inf: pure k-NN.  A NaN distance never enters a list.  count [total] int32; idx [total, max_nn] int32, -1 past count; d2
 * [total, max_nn] f64, +inf past count.  Brute force, hence exact; meant for clouds of up to about 20 000 points, larger ones are merely slow.
 *
 * sga_normals: viewpoints [n_clouds, 3] f64, nullable.  m = count[i].  m < 3, a non-finite coordinate of the point or of a neighbour, or an
 * index outside the cloud: normal (0, 0, 1), status 1, no orientation (Open3D's rule for too few neighbours).  Otherwise: mean = the sum
 * in list order / m; the six covariance entries = the sums of (q - mean)_a (q - mean)_b in list order / m; eigenvectors by 8 cyclic Jacobi
 * sweeps (pairs (0,1), (0,2), (1,2); a pair whose off-diagonal entry is exactly 0 is left alone); normal = the unit eigenvector of the
 * smallest eigenvalue, the lowest column among exactly equal ones.  Orientation: with a viewpoint v negate when n . (v - p) < 0; without
 * one negate so that the component of largest magnitude (lowest axis on ties) is positive.  normals [total, 3] f64, status [total] int32.
 *
 * sga_spfh_counts: counts [total, 33] int32, all zeros when m <= 1.  For list entries k = 1 .. m-1 (entry 0 is taken to be the point
 * itself, as Open3D does), p1 the point, p2 the neighbour, n1 / n2 their normals, dp = p2 - p1, d = sqrt(d2_k):  d == 0 -> (f0, f1, f2) =
 * (0, 0, 0); else a1 = n1.dp / d, a2 = n2.dp / d; if |a1| < |a2|: swap n1 and n2, dp = -dp, f2 = -a2 (Open3D's acos|a1| > acos|a2| up to
 * the rounding of acos), else f2 = a1; v = dp x n1; |v| == 0 -> (0, 0, 0); else v /= |v|, w = n1 x v, f1 = v.n2, f0 = atan2(w.n2, n1.n2).
 * Bins b0 = floor(11 (f0 + pi) / 2 pi), b1 = floor(11 (f1 + 1) / 2), b2 = floor(11 (f2 + 1) / 2), each clamped to [0, 10], a NaN to 0;
 * counts[i, b0], counts[i, 11 + b1], counts[i, 22 + b2] each gain 1.  A neighbour index outside the cloud is skipped, never read.
 *
 * sga_fpfh: with s_x[j] = counts[x, j] * (100.0 / (m_x - 1)) (0 when m_x <= 1), for point i and bin group g (columns 11 g .. 11 g + 10):
 * acc_j = 0, sum_g = 0; for k = 1 .. m-1 ascending, skipping d2_k == 0 and indices outside the cloud, for j ascending within the group:
 * val = s_{idx_k}[j] / d2_k (the SQUARED distance, as in Open3D), sum_g += val, acc_j += val.  Then if sum_g != 0: acc_j *= 100.0 / sum_g.
 * out[i, j] = acc_j + s_i[j].  Each operation rounded on its own, in exactly this order.  out64 [total, 33] f64, nullable; out32
 * [total, ld] f32, ld >= 33 and ld % 4 == 0, the padding columns zero (ld = 36 feeds sga_featnn_search as it is); the f32 values are the
 * round-to-nearest casts of the f64 values. */
int sga_knn_lists(const double* pts, const int32_t* offsets, int n_clouds, int total_points, const int32_t* offsets_host, double r2,
                  int max_nn, int32_t* count, int32_t* idx, double* d2, void* stream);
int sga_normals(const double* pts, const int32_t* offsets, int n_clouds, int total_points, const int32_t* offsets_host,
                const int32_t* count, const int32_t* idx, int max_nn, const double* viewpoints, double* normals, int32_t* status,
                void* stream);
int sga_spfh_counts(const double* pts, const double* normals, const int32_t* offsets, int n_clouds, int total_points,
                    const int32_t* offsets_host, const int32_t* count, const int32_t* idx, const double* d2, int max_nn, int32_t* counts,
                    void* stream);
int sga_fpfh(const int32_t* counts, const int32_t* offsets, int n_clouds, int total_points, const int32_t* offsets_host,
             const int32_t* count, const int32_t* idx, const double* d2, int max_nn, double* out64, float* out32, int ld, void* stream);

/* ---- voxel grid: cells of a packed batch, voxel down-sampling, grid neighbour lists (fp64; csrc/voxel.hip) -------------------------
 * utils/open3d.py:68-76 (voxel_downsample) and an accelerator for sga_knn_lists.  Open3D is not a dependency and equality with its output
 * is not tested: the text below is the definition (tests/voxel_ref.py restates it in numpy).  Clouds are packed back to back as above:
 * pts [total_points, 3] f64, offsets [n_clouds + 1] DEVICE int32, offsets_host (nullable) validated before anything is launched.  The
 * kernels re-check every offset, index and count they read: a bad one makes them do nothing, never read or write out of bounds.  No
 * atomics: every output is a pure function of the input.  Every fp64 operation below is rounded on its own.  Stream-ordered.
 *
 * The grid.  cell [n_clouds] f64 DEVICE: the cell edge h_c of each cloud; cell_host (nullable) is a host copy, refused unless every h_c
 * is > 0 and finite.  A point with a non-finite coordinate is DROPPED: it belongs to no cell, takes no part in the bounds and never
 * enters a voxel.  origin_c[a] = (min over the cloud's kept points of p[a]) - 0.5 * h_c: the min bound minus half a voxel (Open3D's rule
 * as remembered; not tested against it); (0, 0, 0) for a cloud without a kept point.  k[a] = floor((p[a] - origin_c[a]) / h_c): sub,
 * div, floor.  dims_c[a] = k[a] of the cloud's max bound + 1 (0 without a kept point): k is monotone in p, so every kept point has
 * 0 <= k[a] < dims_c[a].  A cloud is valid when h_c > 0 is finite, every k[a] < 65535 and n_clouds <= 32767; otherwise status 2 ("grid
 * too fine"), dims 0, no cells, and nothing of it is read further.  key = cloud << 48 | kx << 32 | ky << 16 | kz (int64, non-negative);
 * a dropped point and every point of a status-2 cloud take the cell (65535, 65535, 65535) of their cloud, so they sort to its end.
 * sga_voxel_keys writes origin [n_clouds, 3] f64, dims [n_clouds, 3] int32, keys [total_points] int64 and status [n_clouds] int32.
 * sga_cloud_bounds writes only the bounds the origin comes from: box [n_clouds, 6] f64 = min xyz | max xyz over each cloud's kept points,
 * +inf | -inf for a cloud without one, and with edge [n_clouds] f64 (nullable) the cell edge at which an occupied cell of a SURFACE
 * spread across the cloud's box holds about per_cell points: with the extents e1 >= e2 >= e3 and n the cloud's point count,
 * sqrt(e1 e2 per_cell / n), e1 per_cell / n for points on a line, never below e1 / 60000, 1 for a cloud without extent.  The edge is a
 * speed choice for sga_knn_lists_grid and never part of a result; its arithmetic is not pinned.
 *
 * order [total_points] int32 is the STABLE ascending argsort of keys, an INPUT of everything below (the 64-bit sort is borrowed: the
 * Python wrapper takes it from torch.sort(keys, stable=True)).  The cloud id is the top field and clouds are packed in ascending order,
 * so the sorted positions of cloud c are exactly [offsets[c], offsets[c + 1]) and the points of a cell come in ascending original index.
 * sga_voxel_cells verifies that in O(n): every entry of a cloud's range lies in the cloud and the pairs (key, index) are strictly
 * increasing along it -- together a proof of the stable permutation.  A cloud that fails gets status 3 and produces nothing (status 2
 * stays 2).  It writes sorted_keys [total_points] int64 (keys[order[t]]; the cloud's dropped key where order[t] is outside the cloud).
 * A sorted position is a HEAD when its point is kept and it is the first of its cloud or its key differs from its predecessor's; voxel
 * ids are the exclusive prefix sum of the heads (a block scan plus one workgroup over the block totals, no atomics), cloud-local after
 * subtracting the cloud's first.  Voxels are therefore numbered in ascending (kx, ky, kz) -- NOT Open3D's hash-map order.
 * voxel_of_point [total_points] int32: the cloud-local voxel of each point, -1 for a dropped point and for clouds of status 2 / 3.
 * voxel_offsets [n_clouds + 1] int32: the prefix of voxels per cloud.  voxel_first [total_points + 1] int32: entry voxel_offsets[c] + v is
 * the sorted position of the head of voxel v of cloud c; the run of a voxel ends where sorted_keys changes or the cloud ends (for all but
 * a cloud's last voxel that is the next entry); entry voxel_offsets[n_clouds] holds total_points, later entries are not written.
 * status [n_clouds] is read (0 / 2 from sga_voxel_keys) and updated.  workspace: sga_voxel_workspace_bytes(n_clouds, total_points).
 *
 * sga_voxel_downsample: voxel g (global id) with sorted run [s, e): sum = 0, then sum += pts[order[t]] for t ascending -- ascending
 * original index --, out_pts[g] = sum / (e - s), out_count[g] = e - s; normals [total_points, 3] f64 (nullable, with out_normals):
 * out_normals[g] is the same mean, NOT re-normalised.  The caller sizes out_pts / out_normals / out_count for total_points voxels;
 * voxel_offsets[n_clouds] of them are written, packed by cloud.  Colours are not carried.
 *
 * sga_knn_lists_grid: count / idx / d2 of sga_knn_lists, bit for bit, for every input and every cell size: the grid decides how much of
 * a cloud is looked at, never what comes out.  Per query, the blocks of cells |k - c|inf <= R, R = 1, 2, 4, 8, 16, are scanned until no point
 * outside the block can enter the list (the proof is at the head of csrc/voxel.hip); a query that stays undecided, a dropped query, and
 * every query of a cloud whose status is not 0 walks its whole cloud as sga_knn_lists does.  cell / origin / dims / status / order /
 * sorted_keys are the arrays of sga_voxel_keys and sga_voxel_cells for the same pts and offsets.  r2 and max_nn as in sga_knn_lists. */
size_t sga_voxel_workspace_bytes(int n_clouds, int total_points);
int sga_cloud_bounds(const double* pts, const int32_t* offsets, int n_clouds, int total_points, const int32_t* offsets_host, double* box,
                     double per_cell, double* edge, void* stream);
int sga_voxel_keys(const double* pts, const int32_t* offsets, int n_clouds, int total_points, const int32_t* offsets_host,
                   const double* cell, const double* cell_host, double* origin, int32_t* dims, int64_t* keys, int32_t* status, void* stream);
int sga_voxel_cells(const int32_t* offsets, int n_clouds, int total_points, const int32_t* offsets_host, const int64_t* keys,
                    const int32_t* order, int64_t* sorted_keys, int32_t* voxel_of_point, int32_t* voxel_offsets, int32_t* voxel_first,
                    int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int sga_voxel_downsample(const double* pts, const double* normals, const int32_t* offsets, int n_clouds, int total_points,
                         const int32_t* offsets_host, const int32_t* order, const int64_t* sorted_keys, const int32_t* voxel_offsets,
                         const int32_t* voxel_first, const int32_t* status, double* out_pts, double* out_normals, int32_t* out_count,
                         void* stream);
int sga_knn_lists_grid(const double* pts, const int32_t* offsets, int n_clouds, int total_points, const int32_t* offsets_host,
                       const double* cell, const double* origin, const int32_t* dims, const int32_t* status, const int32_t* order,
                       const int64_t* sorted_keys, double r2, int max_nn, int32_t* count, int32_t* idx, double* d2, void* stream);

/* ---- cross-cloud nearest neighbour through the support cloud's grid (fp64; csrc/icp.hip) --------------------------------------------
 * The search under ICP refinement and under the geometric score of a transform (Open3D's evaluate_registration): for every query of one
 * cloud, moved by a transform, the nearest point of ANOTHER cloud within a radius, without nq x ns work.  tests/icp_ref.py restates the
 * text below in numpy.
 * pts / offsets / pairs / out_offsets / total_queries / max_queries / offsets_host / pairs_host / squared / out_dist / out_idx: as in
 * sga_nn_search (a job is a (query cloud, support cloud) pair; csrc/pair_jobs.h).  cell / origin / dims / status / order / sorted_keys:
 * the arrays of sga_voxel_keys and sga_voxel_cells for the same pts and offsets (every cloud that is a support has its grid there).
 * transforms [n_pairs, 12] f64 DEVICE, nullable: row-major [R | t] per job, m[0..8] = R, m[9..11] = t (sga_ransac_rigid's model layout).
 * r2 >= 0, +inf: no radius.
 * The moved query: without transforms q' = q.  With them x' = ((m0*x + m1*y) + m2*z) + m9, y' = ((m3*x + m4*y) + m5*z) + m10,
 * z' = ((m6*x + m7*y) + m8*z) + m11, every operation rounded on its own (no FMA).
 * The result: among the support points with d2 <= r2 the one of minimal d2, the LOWEST support-cloud-local index among exactly equal
 * minima; d2 = (dx*dx + dy*dy) + dz*dz, dx = x' - s.x ...: sga_nn_search's arithmetic and its rules -- a NaN never wins, an empty support
 * gives +inf, -1 -- and nothing within r2 gives +inf, -1 as well.  out_dist = d2 when squared != 0, else the correctly rounded sqrt(d2).
 * The grid decides how much of the support is looked at, never what comes out: for every input and every cell size out_dist / out_idx
 * equal, as bit patterns, what sga_nn_search gives on the moved points, masked by d2 <= r2.  Per query the cell coordinate relative to
 * the support's origin / cell is clamped (in fp64) into the support's cell box, the blocks |k - c|inf <= R, R = 1, 2, 4, 8, 16, around the
 * clamped cell are scanned until no point outside the block can win (the proof, also for a centre outside the box, is at the head of
 * csrc/icp.hip) or the block covers the box; a query that stays undecided, a query with a non-finite moved coordinate and every query
 * against a support whose status is not 0 walks the whole support.  One wave per query; no atomics, no workspace, stream-ordered; the
 * kernel re-checks every id, offset and index it reads. */
int sga_nn_search_grid(const double* pts, const int32_t* offsets, int n_clouds, int total_points, const int32_t* pairs, int n_pairs,
                       const int32_t* out_offsets, int total_queries, int max_queries, const int32_t* offsets_host, const int32_t* pairs_host,
                       const double* cell, const double* origin, const int32_t* dims, const int32_t* status, const int32_t* order,
                       const int64_t* sorted_keys, const double* transforms, double r2, int squared, double* out_dist, int32_t* out_idx,
                       void* stream);

/* ---- batched ICP refinement, point-to-point and point-to-plane (fp64; csrc/icp.hip) -------------------------------------------------
 * Open3D's registration_icp loop -- evaluate; then repeat { update, evaluate, stop when both changes are small } -- for every job of a
 * list at once, and with max_iters = 0 its evaluate_registration: fitness, inlier RMSE and the correspondence set of a transform at a
 * distance.  Open3D is not a dependency and equality with its output is not tested: the text below is the definition
 * (tests/icp_ref.py restates it in numpy, with SVD Kabsch and numpy.linalg.solve as the yardstick solvers).
 * Jobs, clouds and grid arrays as in sga_nn_search_grid: job p aligns its query cloud (the source) to its support cloud (the reference).
 * r2: the squared maximal correspondence distance.  method: 0 point-to-point, 1 point-to-plane.  normals [total_points, 3] f64: the
 * normals of every cloud that is a support (method 1; nullable for method 0).  pivot [n_pairs, 3] f64: a point near the job's clouds (the
 * Python layer passes the support cloud's box minimum from sga_cloud_bounds); all sums are taken about it, so that coordinates of order
 * 10^3 cost no digits.  max_iters >= 0; rel_fitness, rel_rmse: the stop thresholds.
 * transform [n_pairs, 12] f64, IN / OUT: row-major [R | t] per job, the initial estimate on entry, the final one on return.
 * Out, per job: fitness, inlier_rmse (f64), iters, status (int32), trace [n_pairs, max_iters + 1, 2] f64 (fitness and RMSE of every
 * evaluation made, NaN after the last), and out_idx / out_d2 [total_queries] laid out by out_offsets: sga_nn_search_grid's outputs
 * (squared distances) for the FINAL transform.
 * Evaluation k = 0, 1, ... of a job: the search with the current transform T; count = #{out_idx >= 0}; fitness = count / nq (0 for an
 * empty query cloud); rmse = sqrt(sum d2 / count), 0 without a pair; both go to trace[k]; iters = k.  The job is done with status 0 when
 * k == max_iters, or when k >= 1 and |fitness - previous| < rel_fitness and |rmse - previous| < rel_rmse.  Otherwise an update U is
 * computed from the pairs and T <- U T (R <- R_U R, t <- R_U t + t_U):
 *   fewer than 3 pairs (method 0) or fewer than 6 (method 1): status 1, the job is done and T is kept.
 *   method 0: U = the least-squares proper rotation + translation of the pairs (x', s), x' the moved query: Horn's quaternion from the 15
 *     moments sum a, sum b, sum a b^T, a = x' - pivot, b = s - pivot (sga_ransac_rigid's solver).
 *   method 1: with n the partner's normal, r = (a - b) . n and J = [a x n, n] (6 entries): (sum J J^T) x = -sum J r by Cholesky without
 *     pivoting; a pivot that is <= 0 or not finite gives status 2, the job is done and T is kept.  R_U = Rz(x2) Ry(x1) Rx(x0),
 *     t_U = (x3, x4, x5) + pivot - R_U pivot.
 *   a non-finite U or U T: status 2, done, T kept.
 * A job whose ids or offsets are out of range on the device: status 3, nothing else of it is written but fitness = rmse = 0, iters = 0.
 * The sums are a fixed fold (csrc/icp.hip: lanes in row order, wave butterfly, waves in order, slices of 1024 query rows counted from the
 * job's first row, ascending): no atomics, two calls give the same bits, and a job in a batch gives the bits of the same job alone.
 * One stream, no host synchronisation inside the call: max_iters + 1 rounds of three kernels (search, accumulate, step); a finished job
 * sets a flag in the workspace and later rounds skip its workgroups.  workspace: sga_icp_workspace_bytes(n_pairs, max_queries). */
size_t sga_icp_workspace_bytes(int n_pairs, int max_queries);
int sga_icp(const double* pts, const int32_t* offsets, int n_clouds, int total_points, const int32_t* pairs, int n_pairs,
            const int32_t* out_offsets, int total_queries, int max_queries, const int32_t* offsets_host, const int32_t* pairs_host,
            const double* cell, const double* origin, const int32_t* dims, const int32_t* grid_status, const int32_t* order,
            const int64_t* sorted_keys, double r2, int method, const double* normals, const double* pivot, int max_iters, double rel_fitness,
            double rel_rmse, double* transform, double* fitness, double* inlier_rmse, int32_t* iters, int32_t* status, double* trace,
            int32_t* out_idx, double* out_d2, void* workspace, size_t workspace_bytes, void* stream);

/* ---- batched RANSAC rigid registration from point correspondences, fp64 -------------------------------------------------------
 * the estimator of src/engine/registration_evaluator.py:129-208 (pygcransac.findRigidTransform with min_iters == max_iters and
 * spatial_coherence_weight == 0: a fixed number of three-point hypotheses, scored against every correspondence, then least-squares refits
 * on the inliers) and of utils/open3d.py:172-201.  Jobs are packed back to back: corr [total_rows, 6] f64, a row = source xyz | reference
 * xyz; offsets [n_jobs + 1]; samples [total_hyp, 3] job-local row indices; hyp_offsets [n_jobs + 1].  These are DEVICE arrays;
 * offsets_host / hyp_offsets_host (nullable) are host copies that, when given, are validated before anything is launched.  max_rows /
 * max_hyp: the largest job (they size the grid; the kernels re-check every offset and sample they read, a bad one makes them do nothing).
 * The samples are an input and no atomics are used: the output is a pure function of the arguments, bit for bit.
 * Hypothesis h: the least-squares proper rotation + translation of its three pairs (Horn's quaternion by Jacobi sweeps); invalid (a
 * repeated or out-of-range index, a non-finite result) -> count 0, never selected.  hyp_count[h] = #{i : |R s_i + t - r_i|^2 <= threshold^2}.
 * Selected: the LOWEST index among the hypotheses with the maximal count.  Then refine_rounds times: least-squares fit over the current
 * inliers, recount, keep it if the count did not drop, else stop.  Per job: transform [4, 4] row-major, column-vector convention
 * (ref ~ R src + t); inlier_count; best_hyp; status 0 = ok, 1 = no model (fewer than 3 rows, no valid hypothesis, best count below 3:
 * identity, count 0, mask 0, best_hyp -1); inlier_mask [total_rows] and inlier_count belong to the final transform.
 * refine_rounds == -1 stops after the scoring: hyp_count is written, the per-job outputs and the mask are left untouched.
 * chunk: rows per scoring workgroup pass; per-chunk counts go to the workspace and are folded in ascending order. */
size_t sga_ransac_workspace_bytes(int n_jobs, int total_hyp, int max_rows, int chunk);
int sga_ransac_rigid(const double* corr, const int32_t* offsets, int n_jobs, int total_rows, const int32_t* samples,
                     const int32_t* hyp_offsets, int total_hyp, int max_rows, int max_hyp, int chunk, const int32_t* offsets_host,
                     const int32_t* hyp_offsets_host, double threshold, int refine_rounds, double* transform, int32_t* inlier_count,
                     int32_t* best_hyp, int32_t* status, unsigned char* inlier_mask, int32_t* hyp_count, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ---- feature-matching RANSAC scored geometrically: hypothesis models and the score of many transforms (fp64; csrc/ransac_geo.hip) ----
 * Open3D's registration_ransac_based_on_feature_matching judges a validated hypothesis by evaluate_registration: a nearest-neighbour
 * search of ALL moved source points in the reference cloud.  These two entries are its device half; the selection between them is
 * utils/registration.py's ransac_geometric_batch.  tests/ransac_geo_ref.py restates the text below in numpy.
 *
 * sga_ransac_models: corr / offsets / samples / hyp_offsets / total_rows / total_hyp / max_hyp / offsets_host / hyp_offsets_host as in
 * sga_ransac_rigid.  Out, per hypothesis h (packed by hyp_offsets): models [total_hyp, 12] f64, row-major [R | t], m[0..8] = R,
 * m[9..11] = t -- sga_ransac_rigid's three-point model: the least-squares proper rotation + translation of the three sampled pairs about
 * the first of them, Horn's quaternion by at most 10 cyclic Jacobi sweeps, the same validity rules; valid [total_hyp] int32; resid2
 * [total_hyp] f64 = the largest of the three sampled rows' |R s + t - r|^2, taken in sga_nn_search_grid's arithmetic:
 * x' = ((m0*x + m1*y) + m2*z) + m9 (y', z' with rows 1, 2), dx = x' - r.x ..., d2 = (dx*dx + dy*dy) + dz*dz, every operation rounded on its
 * own (no FMA), so that a host recomputes resid2 bit for bit from the downloaded model and rows.  Invalid -- a repeated or out-of-range
 * index, a non-finite model, a NaN residual --: valid = 0, resid2 = +inf, all twelve model entries NaN.  One lane per hypothesis; no
 * atomics, no workspace, stream-ordered: the outputs are a pure function of the inputs.  The kernel re-checks every offset and index it
 * reads; a job whose offsets are out of range on the device writes nothing.  With n_jobs, total_hyp or max_hyp 0 nothing is launched.
 *
 * sga_score_transforms_grid: pts / offsets / n_clouds / total_points / pairs / n_pairs / max_queries / offsets_host / pairs_host and
 * cell / origin / dims / status / order / sorted_keys as in sga_nn_search_grid (a job is a (query cloud, support cloud) pair; there is
 * no out_offsets: nothing is written per query).  transforms [n_pairs, 12] f64 DEVICE, required: job p's [R | t].  live [n_pairs] int32
 * DEVICE, nullable: a job with live[p] == 0 is not searched.  r2 >= 0, +inf: no radius.
 * Out: count [n_pairs] int32 = the number of queries of job p for which sga_nn_search_grid (same arrays, same transform, same r2) returns
 * an index >= 0; sum_d2 [n_pairs] f64 = the sum of their d2, in this fixed order: a slice is 1024 query rows counted from the job's first
 * row; wave w = 0..3 of a slice's workgroup adds the d2 of rows w, w + 4, w + 8, ... of the slice in ascending order, starting from +0.0;
 * the four wave sums are added in order, starting from wave 0's; the slice sums are added in ascending order, starting from +0.0.  Every
 * addition is one fp64 rounding.  A job with live == 0, or whose ids or offsets are out of range on the device, gets count 0 and sum_d2 0.
 * The search -- moved query, clamp, blocks R = 1, 2, 4, 8, 16, stop rule, whole walk -- is sga_nn_search_grid's, unchanged, one wave per
 * query; the grid decides how much of the support is looked at, never what comes out.  No atomics: count and sum_d2 have the same bits
 * in two calls, for a job alone or in a batch, and for every cell size.  Two launches (search + fold of a slice; fold of the slices),
 * stream-ordered, no synchronisation.  workspace: sga_score_transforms_workspace_bytes(n_pairs, max_queries) = 16 bytes per (job, slice
 * of the longest query cloud); it need not be zeroed.  A job list with ceil(max_queries / 1024) x n_pairs >= 2^24 workgroups (2^32 threads
 * in one launch; far below the point where the count would overflow an int) is refused with a message before anything is launched. */
int sga_ransac_models(const double* corr, const int32_t* offsets, int n_jobs, int total_rows, const int32_t* samples,
                      const int32_t* hyp_offsets, int total_hyp, int max_hyp, const int32_t* offsets_host, const int32_t* hyp_offsets_host,
                      double* models, int32_t* valid, double* resid2, void* stream);
size_t sga_score_transforms_workspace_bytes(int n_pairs, int max_queries);
int sga_score_transforms_grid(const double* pts, const int32_t* offsets, int n_clouds, int total_points, const int32_t* pairs, int n_pairs,
                              int max_queries, const int32_t* offsets_host, const int32_t* pairs_host, const double* cell,
                              const double* origin, const int32_t* dims, const int32_t* status, const int32_t* order,
                              const int64_t* sorted_keys, const double* transforms, const int32_t* live, double r2, int32_t* count,
                              double* sum_d2, void* workspace, size_t workspace_bytes, void* stream);

/* ---- batched subscan generation: frame visibility, frustum walk, per-object counts (fp64 tests, integer walk) ----------------------
 * replaces the per-frame loop of preprocessing/scan3r/subgenscan3r.py:188-234: utils/point_cloud.py:112-134 get_visible_pts_from_cam_pose
 * for every frame, the running OR of the masks with a subscan closed whenever the union reaches the point budget, and the per-object
 * visible-point counts of gen_scene_graph (:51-85).  Scans are packed back to back: pts [total_points, 3] f32 (the ply vertices as stored)
 * / pt_off [n_scans + 1]; w2c [total_frames, 12] f64 (rows 0-2 of the world-to-camera matrix, row-major) / fr_off [n_scans + 1]; intr
 * [n_scans, 6] f64 = fx, fy, cx, cy, u_max, v_max.  Scan s owns a bit matrix of F_s rows by W_s = ceil(N_s / 64) 64-bit words that starts
 * at word vis_off[s] of a [total_words] array (vis_off [n_scans + 1] int64, the prefix sum of F_t * W_t); bit p % 64 of word p / 64 of a row
 * is point p, the padding bits of the last word are 0.  These are DEVICE arrays; pt_off_host / fr_off_host / vis_off_host (nullable) are host
 * copies that, when given, are validated before anything is launched.  max_points / max_frames: the largest scan (they size the grid; the
 * kernels re-check every offset they read, a bad one makes them do nothing).  Stream-ordered, no allocation, no synchronisation.
 * sga_frame_visibility writes the bit matrices.  Per (frame, point), every fp64 operation rounded on its own (no FMA), x, y, z the f32
 * vertex widened to f64:  X = ((x*m00 + y*m01) + z*m02) + m03 (Y, Z with rows 1, 2);  r = (Z != 0) ? 1.0 / Z : 1.0 (correctly rounded);
 * u = (X*r)*fx + cx, v = (Y*r)*fy + cy;  visible = (Z > 0) && (u >= 0) && (u <= u_max) && (v >= 0) && (v <= v_max).  A NaN anywhere gives
 * invisible.  (The reference compares the first image coordinate with the HEIGHT and the second with the WIDTH; its callers here pass
 * u_max = height, v_max = width.)
 * sga_subscan_walk, per scan with max_pts[s]:  cur = 0; k = 0; for f in 0 .. F-1: cur |= vis[f]; cum[f] = cur; c = popcount(cur);
 * frame_count[f] = c; if c >= max_pts: seg_end[k] = f; seg_count[k] = c; k += 1; cur = 0.  n_seg[s] = k (the unclosed tail is discarded, as
 * in the reference).  cum may be vis itself (in place): subscan k's mask is then row seg_end[k].  seg_end / seg_count / frame_count are
 * [total_frames], scan s's entries start at fr_off[s]; seg_end is scan-local.  A scan with N == 0 or F == 0 gets n_seg = 0 and nothing else.
 * sga_subscan_object_counts: rows [n_rows, 2] = (scan, scan-local frame row) of the matrix `bits`; slot [total_points] the dense object slot
 * of every point in [0, n_slots) (a slot outside that range is not counted); counts [n_rows, n_slots] = set bits of the row per slot,
 * zeroed by the call.  Integer atomics (a workgroup-private histogram up to sga_subscan_lds_slots() slots, global atomics above): exact and
 * independent of the order of execution. */
int sga_subscan_lds_slots(void);
int sga_frame_visibility(const float* pts, const int32_t* pt_off, const double* w2c, const int32_t* fr_off, const double* intr,
                         const int64_t* vis_off, int n_scans, int total_points, int total_frames, int64_t total_words, int max_points,
                         int max_frames, const int32_t* pt_off_host, const int32_t* fr_off_host, const int64_t* vis_off_host,
                         uint64_t* vis, void* stream);
int sga_subscan_walk(const uint64_t* vis, uint64_t* cum, const int32_t* pt_off, const int32_t* fr_off, const int64_t* vis_off,
                     const int32_t* max_pts, int n_scans, int total_points, int total_frames, int64_t total_words,
                     const int32_t* pt_off_host, const int32_t* fr_off_host, const int64_t* vis_off_host, int32_t* seg_end,
                     int32_t* seg_count, int32_t* frame_count, int32_t* n_seg, void* stream);
int sga_subscan_object_counts(const uint64_t* bits, const int32_t* pt_off, const int32_t* fr_off, const int64_t* vis_off, int n_scans,
                              int total_points, int total_frames, int64_t total_words, int max_points, const int32_t* rows, int n_rows,
                              const int32_t* slot, int n_slots, const int32_t* pt_off_host, const int32_t* fr_off_host,
                              const int64_t* vis_off_host, const int32_t* rows_host, int32_t* counts, void* stream);

/* ---- scene-graph records (preprocessing/scan3r/preprocess.py:40-211 process_scan and the two bag-of-words passes :280-361) ----
 * Integers only: every output is a pure function of the input (integer atomics and prefix sums in index order).  Scans are packed back to
 * back: slot [sum N] int32 = each point's dense object slot within its scan (np.unique(objectId, return_inverse=True)[1]; a value outside
 * the scan's slot range, e.g. -1, belongs to no object), pt_off / slot_off [S + 1] the point and slot ranges.  *_host: host copies,
 * validated before any launch (nullable for sga_object_counts and sga_bow_counts, required elsewhere); the kernels re-derive their ranges
 * from the device arrays and do nothing on a bad one.  Caller-owned buffers, caller's stream, no synchronisation.
 *
 * sga_object_counts: counts [sum slots] = points per slot (zeroed by the call); an LDS histogram up to sga_scenegraph_lds_slots() slots per
 * scan, global integer atomics above.
 *
 * sga_object_partition: the stable split.  dest_off [sum slots]: the start of the slot's points in the packed output, -1 = dropped;
 * counts_host: what sga_object_counts returned.  perm [n_kept_points] int32 (scan-local point index) and pts_out [n_kept_points, 3] f32 with
 * perm[dest_off[k] : dest_off[k] + counts[k]] == flatnonzero(slot_s == k): ascending point order, from per-tile histograms
 * (sga_scenegraph_tile() points per tile), an exclusive scan over tiles in tile order and an in-tile ballot rank -- never from the arrival
 * order of an atomic.  At most sga_scenegraph_lds_slots() slots per scan; overlapping or out-of-range destination ranges are refused.
 * ws: sga_object_partition_ws_bytes(n_scans, max_points, max_slots) bytes.
 *
 * sga_graph_complete: one workgroup per graph; node_off / pair_off / trip_off / edge_off [G + 1] int32 prefix arrays.  Graph g has
 * N = diff(node_off) nodes, its listed pairs [P, 2] (graph-local, list order) at pairs + 2 pair_off[g], the relation ids of its listed
 * triples [Tr >= P] at rels + trip_off[g], and room for diff(edge_off) >= P + N (N - 1) edges.  edges [sum, 2] int64: the listed pairs,
 * then every ordered pair (i, j), i != j, that is not listed, row-major; n_edges [G]; bow [sum N, V] int32 (zeroed by the call):
 * bow[edges[idx][0], rel(idx)] += 1 for idx < n_edges, rel(idx) = rels[idx] for idx < Tr, else none_id -- the edge index applied to the
 * TRIPLES list, as the reference does (:303-306), so a pair listed with two relations shifts every later edge by one.  N at most
 * sga_graph_max_nodes() (the adjacency bit matrix and one counter per row fit 64 KiB of LDS).
 *
 * sga_bow_counts: out [T, V] int32 (zeroed by the call), out[rows[i], cols[i]] += 1 for i < n; the host check refuses an entry outside. */
int sga_scenegraph_lds_slots(void);
int sga_scenegraph_tile(void);
int sga_graph_max_nodes(void);
int sga_object_counts(const int32_t* slot, const int32_t* pt_off, const int32_t* slot_off, int n_scans, int total_points, int total_slots,
                      int max_points, const int32_t* pt_off_host, const int32_t* slot_off_host, int32_t* counts, void* stream);
size_t sga_object_partition_ws_bytes(int n_scans, int max_points, int max_slots);
int sga_object_partition(const float* pts, const int32_t* slot, const int32_t* pt_off, const int32_t* slot_off, const int32_t* dest_off,
                         int n_scans, int total_points, int total_slots, int max_points, int max_slots, int n_kept_points,
                         const int32_t* pt_off_host, const int32_t* slot_off_host, const int32_t* dest_off_host, const int32_t* counts_host,
                         int32_t* perm, float* pts_out, void* ws, size_t ws_bytes, void* stream);
int sga_graph_complete(const int32_t* node_off, const int32_t* pair_off, const int32_t* trip_off, const int32_t* edge_off, int n_graphs,
                       const int32_t* pairs, const int32_t* rels, int none_id, int V, const int32_t* node_off_host,
                       const int32_t* pair_off_host, const int32_t* trip_off_host, const int32_t* edge_off_host, const int32_t* pairs_host,
                       const int32_t* rels_host, int64_t* edges, int32_t* n_edges, int32_t* bow, void* stream);
int sga_bow_counts(const int32_t* rows, const int32_t* cols, int n, int T, int V, const int32_t* rows_host, const int32_t* cols_host,
                   int32_t* out, void* stream);

/* Wide tables (Dp > 128) of sga_loss_neg_grad: one anchor-owner sweep writes c_ij = dL/dS_ij to a caller-owned stash (anchor-row blocks
 * sized to stash_floats; sga_loss_neg_grad_wide_floats() = everything in one block), both gradients are GEMMs on it: the K = Dp
 * similarity tile is computed once instead of 2 x ceil(Dp / 320) times.  Same results as sga_loss_neg_grad up to fp32 summation order. */
size_t sga_loss_neg_grad_wide_floats(int A, int J1, int J2);
int sga_loss_neg_grad_wide(const float* Z, int Dp, int A, int J1, int J2, float tau0, float tau1, const double* gs8, float* dZ,
                           float* stash, size_t stash_floats, void* stream);

/* fp16-input / fp32-accumulate variant of the two functions above for WIDE tables (BASELINE.json configs[4]: 1024-d embeddings,
 * "similarity GEMM at fp16"); opt-in from Python (ops.set_mfma_mode('f16')), tolerance 1e-2 on gradients (tests/test_c5_gpu.py).
 * sga_wide16_prepare: packed normalised table Z fp32 [2A+J1+J2][Dp] -> Zh fp16 (same layout) and ZhT fp16 [Dp][sga_wide16_ldt()]
 * (transposed; every segment X1|X2|N1|N2 starts at a multiple of 8 columns).  sums8 / gs8 as in sga_loss_neg_sums / _grad.
 * stash: caller-owned workspace of stash_bytes (sga_loss_neg_grad_f16_bytes() = the whole batch in one pass; less -> anchor-row blocks). */
long sga_wide16_ldt(int A, int J1, int J2);
int sga_wide16_prepare(const float* Z, int Dp, int A, int J1, int J2, void* Zh, void* ZhT, void* stream);
/* [a_lo, a_hi): the anchor shard this process owns (0, A on one GPU; a_lo a multiple of 8 for the gradient) -- the shard's anchors against ALL
 * negatives: partial sums8 (all-reduced by the caller), dZ complete for the shard's anchor rows and partial for the negatives' rows. */
int sga_loss_neg_sums_f16(const void* Zh, int Dp, int A, int J1, int J2, float tau0, float tau1, double* sums8, int a_lo, int a_hi, void* stream);
size_t sga_loss_neg_grad_f16_bytes(int A, int J1, int J2);
int sga_loss_neg_grad_f16(const void* Zh, const void* ZhT, int Dp, int A, int J1, int J2, float tau0, float tau1, const double* gs8,
                          float* dZ, void* stash, size_t stash_bytes, int a_lo, int a_hi, void* stream);
/* sga_loss_stash_grad for a wide table in the same mode (replaces the two fp32 GEMMs; the autograd of src/aligner/losses.py:6,50-57,81-94
 * through S = X1 X2^T): dZ[A + j] += sum_i M1[j, i] Z[a_lo + i], dZ[a_lo + i] += sum_j M1[j, i] Z[A + j] with the coefficients as fp16 of
 * 2^e M1 (2^e: the power of two that puts the block's largest magnitude into [2^13, 2^14), found by a max pass, undone exactly at the end),
 * the rows from ZhT (sga_wide16_prepare), fp32 accumulate.  a_lo must be a multiple of 8.  ws: sga_loss_stash_grad_f16_bytes(A, a_hi - a_lo). */
size_t sga_loss_stash_grad_f16_bytes(int A, int ns);
int sga_loss_stash_grad_f16(const float* M1, const void* ZhT, int Dp, int A, int J1, int J2, float* dZ, int a_lo, int a_hi,
                            void* ws, size_t ws_bytes, void* stream);

/* ---- scalar head of OverallLoss -----------------------------------------------------------------------
 * replaces the one-element arithmetic of src/aligner/losses.py:114-152 + CustomMultiLossLayer.forward :28-34 on the raw terms
 * sums = [S_icl[M+1] | S_ial_a[M] | S_ial_b[M]] (doubles) returned by the loss kernels:
 *   out = [loss, icl_loss_unimodal, icl_loss_multimodal, ial_loss]   (doubles);  inv_a2 = 1 / A^2, z_ial / alpha = IALLoss zoom / alpha,
 *   zoom = cfg.loss.zoom.  bwd: gout[4] = dL/d(out) -> dsums [3M+1] (type of sums), dlv_ial / dlv_icl [M] floats (the two log_vars). */
int sga_loss_head_fwd(const void* sums, int sums_f64, const float* lv_ial, const float* lv_icl, int M, double inv_a2,
                      double z_ial, double alpha, double zoom, double* out, void* stream);
int sga_loss_head_bwd(const double* gout, const void* sums, int sums_f64, const float* lv_ial, const float* lv_icl, int M,
                      double inv_a2, double z_ial, double alpha, double zoom, void* dsums, float* dlv_ial, float* dlv_icl,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SGALIGNER_HIP_H */
