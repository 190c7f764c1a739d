/*
 * simamba.h -- C ABI of libsimamba_hip.so, the MI355X (gfx950) implementation of the
 * SI-Mamba hot path: selective scan (fwd+bwd), causal depthwise conv1d (fwd+bwd) and
 * the k-NN graph-Laplacian eigen-ordering.
 *
 * The reference (denix56/SI-Mamba) is pure Python; the native code on this path lives in
 * un-vendored wheels.  Each entry point below names the reference call site whose native
 * callee it replaces (paths relative to the reference repo):
 *
 *   simamba_selective_scan_fwd/bwd   selective_scan_cuda.fwd/bwd of mamba-ssm, reached from
 *                                    models/block.py:72 (self.mixer(...)) with the mixer built
 *                                    at models/point_mamba.py:162.
 *   simamba_causal_conv1d_fwd/bwd    causal_conv1d_cuda.causal_conv1d_fwd/bwd of causal-conv1d,
 *                                    same call site (inside the mixer).
 *   simamba_xdt_proj_fwd             the x_proj / dt_proj GEMM pair of the same mixer (cuBLAS calls inside
 *                                    upstream's mamba_inner_fn).
 *   simamba_add_layer_norm_fwd/bwd   the Add -> LayerNorm of models/block.py:56-60 (torch ops there); the _ex
 *                                    forms also take RMSNorm (mamba-ssm's Triton kernel upstream).
 *   simamba_out_proj_add_ln_fwd      out_proj of the mixer + that Add -> LayerNorm (or RMSNorm), one kernel (bf16).
 *   simamba_in_proj_fwd              in_proj of the same mixer (a cuBLAS GEMM upstream), fp32 and bf16.
 *   simamba_selective_scan_dt_fwd/bwd  the scan with delta formed in the kernel (same call site, bf16 path).
 *   simamba_knn_graph                models/point_mamba.py:620-661 and :664-715
 *                                    (create_graph_from_centers / ..._feature_space_...).
 *   simamba_laplacian_topk[_ex]      models/point_mamba.py:717-761 and :764-814
 *                                    (per-sample torch.linalg.eigh loop, cuSOLVER underneath).
 *   simamba_spectral_topk            the two above fused: centres -> top-k eigenpairs + orders.
 *   simamba_argsort_rows             the torch.sort of models/point_mamba.py:820.
 *   simamba_curve_order              no call site: Hilbert / Z-order serialisations of the centres, the baseline the
 *                                    reference's method is compared with, as a second producer of (B,k,G) orders.
 *   simamba_farthest_point_sample    pytorch3d.ops.sample_farthest_points, models/point_mamba.py:93.
 *   simamba_augment_points           tools/runner_finetune.py:191-194 (fps_idx[:, choice], gather_operation) and the
 *                                    transforms of datasets/data_transforms.py, one launch per batch.
 *   simamba_dataset_fetch            the torch DataLoader of tools/builder.py over the datasets/ classes and
 *                                    part_segmentation/dataset.py: shuffle, per-item sampling, pc_norm, collate.
 *   simamba_svm_ovo_fit/_vote        sklearn.svm.SVC(C=0.01, kernel='linear') (libsvm) of
 *                                    tools/runner_pretrain.py:66-77.
 *   simamba_tsne_calibrate/_run      sklearn.manifold.TSNE(n_components=2, init='pca') of
 *                                    tools/runner_finetune.py:605-612, with the exact gradient.
 *   simamba_optim_adamw_step         clip_grad_norm_ + torch.optim.AdamW.step of tools/runner_finetune.py:200-215 and
 *                                    timm's per-epoch CosineLRScheduler of tools/builder.py:87-95, three launches.
 *
 * Conventions
 *   - Plain pointers and sizes only.  All pointers are DEVICE pointers unless noted.
 *   - The caller owns every buffer (incl. workspace); the library allocates nothing and keeps
 *     no mutable global state.  Calls only enqueue work on `stream` (a hipStream_t passed as
 *     void*); no device-wide synchronisation, no default-stream use, no hipSetDevice.
 *   - Return 0 on success; <0 = argument error detected before any launch (SIMAMBA_E_*);
 *     >0 = hipError_t reported by the runtime for the launch.  simamba_strerror() decodes both.
 *   - Tensors are contiguous in the layouts stated per function, except where a stride argument
 *     (in ELEMENTS) is given: z / dz / conv x / conv dx may be batch-strided views (e.g. halves of
 *     the mixer's (batch, 2*dim, seqlen) in_proj output), and B, C may be read through arbitrary
 *     (batch, state, time) strides (e.g. straight out of the (batch, seqlen, R+2N) x_proj output).
 *     A stride of 0 means "contiguous default".
 *   - io_dtype: SIMAMBA_F32 or SIMAMBA_BF16 for activation-sized tensors; all state,
 *     accumulation and parameter gradients are fp32.  The exceptions are the simamba_svm_ovo_* family, which is
 *     float64 throughout, and the fp64 sums and outputs of the simamba_tsne_* family (both stated there).
 */
#ifndef SIMAMBA_H_
#define SIMAMBA_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIMAMBA_ABI_VERSION 9

#define SIMAMBA_F32  0
#define SIMAMBA_BF16 1

#define SIMAMBA_OK            0
#define SIMAMBA_E_NULLPTR    -1
#define SIMAMBA_E_SHAPE      -2
#define SIMAMBA_E_DTYPE      -3
#define SIMAMBA_E_DSTATE     -4   /* dstate must be in [1,16] */
#define SIMAMBA_E_WIDTH      -5   /* conv width must be in [2,4] */
#define SIMAMBA_E_WORKSPACE  -6
#define SIMAMBA_E_GROUPS     -7   /* G in [2,128] (simamba_laplacian_topk) or [2,512] (graph, _ex, fused),
                                     knn + 1 <= min(G,32), k (+1) <= G (<= 8 above 128), F in [1,64] */
#define SIMAMBA_E_ALIGN      -8
#define SIMAMBA_E_VARIANT    -9   /* unknown forward-scan variant, or one the shape / alignment cannot take; unknown
                                     flag bits */
#define SIMAMBA_E_BIAS       -10  /* SIMAMBA_NORM_RMS with a bias / beta (RMSNorm has none: pass NULL) */

/* timesteps per scan chunk; simamba_scan_num_chunks(L) = ceil(L / chunk) */
#define SIMAMBA_SCAN_CHUNK 128

/*
 * State checkpoints handed from the forward to the backward (`x_ckpt`, `ckpt_step` of both calls; 0 = _ROW):
 *   SIMAMBA_SCAN_CKPT_ROW  (batch, dim, nchunks, dstate): state at the end of every 128-step chunk; written by every
 *                          forward kernel, read by the row-scan backward (any shape).
 *   SIMAMBA_SCAN_CKPT_SEQ  (batch, ceil(seqlen / 16), dim, 16): state after every 16th step; written by the
 *                          lanes-per-channel forward kernels, read by the sequential backward (dstate == 16,
 *                          dim % 64 == 0, delta_softplus, 16-byte aligned rows and B / C packs, tensors below 2^30
 *                          elements; anything else returns SIMAMBA_E_VARIANT).
 * simamba_scan_ckpt_step() is the library's own choice for a shape (host arithmetic only; the caller still has to
 * meet the alignment rules above or pass _ROW: simamba_scan_seq_applicable() answers that for a set of operands); simamba_scan_ckpt_floats() the size of x_ckpt in floats (0: none
 * needed, x_ckpt may be NULL).  The choice is _SEQ from 49 152 rows (batch * dim) on, and, for fp32 I/O, from
 * 36 864 rows on when seqlen >= 1024 (a mixer that runs on 48 .. 60 samples of a batch of 64: measured,
 * csrc/scan_fwd.hip; bf16 and shorter sequences were not measured there and keep the line).
 */
#define SIMAMBA_SCAN_CKPT_ROW 128
#define SIMAMBA_SCAN_CKPT_SEQ 16

int         simamba_abi_version(void);
const char* simamba_strerror(int rc);           /* host string, static storage */
int         simamba_scan_num_chunks(int seqlen);
/* the forward kernel SIMAMBA_SCAN_AUTO picks for (batch, dim) when the operands qualify for all of them (one of the
 * SIMAMBA_SCAN_* values below; host-side arithmetic only, no GPU work): what a profile's kernel name should be */
int         simamba_scan_fwd_auto_variant(int batch, int dim);
int         simamba_scan_ckpt_step(int batch, int dim, int seqlen, int dstate, int io_dtype);
long long   simamba_scan_ckpt_floats(int batch, int dim, int seqlen, int dstate, int ckpt_step);
/* 1 when simamba_selective_scan_fwd (x_ckpt given, ckpt_step _SEQ, variant AUTO) and simamba_selective_scan_bwd(_ex)
 * with _SEQ would both take these operands, 0 when either would answer SIMAMBA_E_VARIANT: what a caller asks before it
 * allocates 16-step checkpoints (pass _ROW where the answer is 0).  Host arithmetic only, nothing is launched or
 * dereferenced; the answer is built from the predicates the two entry points themselves evaluate.
 *   act_addr_or : bitwise OR of the addresses of every activation-sized operand of both calls (u, delta, out, z,
 *                 dout, du, ddelta, dz) and of x_ckpt: each has to lie on a 16-byte boundary
 *   A_addr, B_addr, C_addr : addresses of A, B and C (B / C: a pack = 4 elements of io_dtype; A: 16 bytes)
 *   strides     : in elements, as in the two calls; 0 => the contiguous default
 * (still ABI version 9: a symbol added, none changed) */
int         simamba_scan_seq_applicable(int batch, int dim, int seqlen, int dstate, int io_dtype, int delta_softplus,
                                        int has_z, size_t act_addr_or, size_t A_addr, size_t B_addr, size_t C_addr,
                                        long long z_bstride, long long dz_bstride, long long bc_bstride,
                                        long long bc_nstride, long long bc_tstride);

/*
 * Selective scan forward.
 *   u, delta, z, out : (batch, dim, seqlen)  io_dtype      z may be NULL (no gating)
 *   A                : (dim, dstate) fp32                   (already -exp(A_log))
 *   B, C             : (batch, dstate, seqlen) io_dtype, element (b,n,t) at b*bc_bstride + n*bc_nstride
 *                      + t*bc_tstride (all three 0 => contiguous (batch, dstate, seqlen))
 *   z_bstride        : elements between consecutive batch samples of z (0 => dim*seqlen)
 *   D, delta_bias    : (dim) fp32, may be NULL
 *   x_ckpt, ckpt_step: state checkpoints for the backward (layouts above) or NULL: required by the backward
 *                      when simamba_scan_ckpt_floats() > 0.  With _SEQ the forward runs a lanes-per-channel kernel
 *                      (SIMAMBA_E_VARIANT if the operands cannot take one or `variant` names the row-scan kernel).
 *   last_state       : (batch, dim, dstate) fp32 or NULL.
 *   variant          : SIMAMBA_SCAN_AUTO in production: the library picks the kernel from the shape (no
 *                      environment variables, no global state).  The explicit values select one kernel for
 *                      benchmarks and parity tests: ROWSCAN (16 lanes per row, any shape), LPC2 / LPC4 (2 / 4
 *                      lanes per channel, 32-step chunks; need dstate == 16, 16-byte aligned rows and tensors
 *                      below 2^30 elements, else SIMAMBA_E_VARIANT), MIX (one launch with the first channels of
 *                      every sample on 2 and the last ones on 4 lanes per channel, for shapes whose 2-lane launch
 *                      leaves at most half a round of waves over, e.g. batch * dim = 49 152; else SIMAMBA_E_VARIANT).
 *                      All variants compute the same function.
 *   out = (scan(u, softplus?(delta + delta_bias), A, B, C) + D*u) * silu(z)
 */
#define SIMAMBA_SCAN_AUTO    0
#define SIMAMBA_SCAN_ROWSCAN 1
#define SIMAMBA_SCAN_LPC2    2
#define SIMAMBA_SCAN_LPC4    4
#define SIMAMBA_SCAN_MIX     6
int simamba_selective_scan_fwd(const void* u, const void* delta, const float* A,
                               const void* B, const void* C, const float* D, const void* z,
                               const float* delta_bias, void* out, float* x_ckpt,
                               float* last_state, int batch, int dim, int seqlen, int dstate,
                               int io_dtype, int delta_softplus, long long z_bstride,
                               long long bc_bstride, long long bc_nstride, long long bc_tstride,
                               int ckpt_step, int variant, void* stream);

/*
 * Selective scan backward.  Inputs as forward (+ dout, and x_ckpt / ckpt_step exactly as given to the
 * forward; ckpt_step selects the kernel: _ROW the row-scan backward, _SEQ the sequential one).
 * du, ddelta, dz : io_dtype (dz NULL iff z NULL).
 * dA (dim,dstate), dB, dC (batch,dstate,seqlen), dD, ddelta_bias (dim): fp32; the library
 * zeroes them on `stream` and then accumulates (float atomics: last-bit run-to-run jitter; see the
 * _ex form below for the deterministic alternative).
 * Not one byte outside these five spans is written: spans that are exactly adjacent in memory
 * (one ends where the next begins) are cleared by a single memset node, all others one by one.
 * dD / ddelta_bias may be NULL when D / delta_bias are NULL.  dB / dC are always contiguous
 * (batch, dstate, seqlen); z, dz and B, C take strides as in the forward.
 */
int simamba_selective_scan_bwd(const void* u, const void* delta, const float* A,
                               const void* B, const void* C, const float* D, const void* z,
                               const float* delta_bias, const void* dout, const float* x_ckpt,
                               void* du, void* ddelta, float* dA, float* dB, float* dC,
                               float* dD, void* dz, float* ddelta_bias,
                               int batch, int dim, int seqlen, int dstate,
                               int io_dtype, int delta_softplus, long long z_bstride,
                               long long dz_bstride, long long bc_bstride, long long bc_nstride,
                               long long bc_tstride, int ckpt_step, void* stream);

/*
 * Deterministic backward (flags of the *_ex backward entry points; 0 = the plain entry point, bit for bit).
 *   SIMAMBA_BWD_DETERMINISTIC: no float atomics.  Every workgroup stores its partial sums to `workspace` and a
 *   fixed-order sum pass (ascending partial index, fp32) writes the parameter gradients -- dA, dB, dC, dD, ddelta_bias
 *   of the scan, dw, dbias of the conv -- WHOLE, so the result is bitwise reproducible run to run for the same inputs,
 *   shape and device.  Written: exactly the spans the plain call writes (no memset is issued: the sum pass stores
 *   every element) plus the first *_workspace_floats() floats of `workspace` (scratch, contents undefined afterwards).
 *   workspace: device memory, 16-byte aligned (else SIMAMBA_E_ALIGN), at least *_workspace_floats() floats (else, or
 *   NULL, SIMAMBA_E_WORKSPACE); unknown flag bits: SIMAMBA_E_VARIANT.  All three checks precede any launch.
 *   *_workspace_floats(): the size for a shape (host arithmetic only); 0 for flags == 0 (workspace may be NULL);
 *   a negative SIMAMBA_E_* for arguments the backward would refuse.  ckpt_step as given to the backward (0 = _ROW;
 *   the dt form always uses _SEQ).
 */
#define SIMAMBA_BWD_DETERMINISTIC 1
long long simamba_scan_bwd_workspace_floats(int batch, int dim, int seqlen, int dstate, int ckpt_step, int flags);
int simamba_selective_scan_bwd_ex(const void* u, const void* delta, const float* A,
                                  const void* B, const void* C, const float* D, const void* z,
                                  const float* delta_bias, const void* dout, const float* x_ckpt,
                                  void* du, void* ddelta, float* dA, float* dB, float* dC,
                                  float* dD, void* dz, float* ddelta_bias,
                                  int batch, int dim, int seqlen, int dstate,
                                  int io_dtype, int delta_softplus, long long z_bstride,
                                  long long dz_bstride, long long bc_bstride, long long bc_nstride,
                                  long long bc_tstride, int ckpt_step, int flags, float* workspace,
                                  long long workspace_floats, void* stream);

/*
 * The mixer's scan with delta formed INSIDE the scan kernels (no (batch, dim, seqlen) delta tensor exists): what
 * upstream's mamba_inner_fn computes between x_proj and out_proj, reached from models/block.py:72.
 *   u      : (batch, dim, seqlen) io_dtype -- the conv output
 *   xdbl   : (batch, seqlen, dt_rank + 2 * 16) io_dtype, token-major -- the x_proj output [dt | B_t | C_t]; element
 *            (b, t, s) at b * xdbl_bstride + t * xdbl_tstride + s (0 => contiguous)
 *   wdt    : (dim, dt_rank) io_dtype -- dt_proj.weight
 *   delta[b, d, t] = sum_r wdt[d, r] * xdbl[b, t, r] on the matrix pipe, with the instruction and k order of
 *   simamba_xdt_proj_fwd: bit for bit the tensor that call would have stored (bf16: rounded to bf16 like it), then
 *   out = (scan(u, softplus(delta + delta_bias), A, B_t, C_t) + D * u) * silu(z) exactly as simamba_selective_scan_fwd.
 * Lanes-per-channel kernels only: dstate == 16, z required, dt_rank % 4 == 0 (bf16: % 8), 4 <= dt_rank <= 24, 16-byte
 * aligned rows; anything else returns SIMAMBA_E_VARIANT / _SHAPE and the caller materialises delta
 * (simamba_xdt_proj_fwd + simamba_selective_scan_fwd).  x_ckpt / ckpt_step / variant / last_state as in
 * simamba_selective_scan_fwd (variant: AUTO, LPC2, LPC4 or MIX).
 * Backward: the sequential kernel (16-step checkpoints of the forward, SIMAMBA_SCAN_CKPT_SEQ; dim % 64 == 0); outputs
 * and accumulators as simamba_selective_scan_bwd, ddelta = gradient w.r.t. the delta formed above.
 */
int simamba_selective_scan_dt_fwd(const void* u, const void* xdbl, const void* wdt, const float* A, const float* D,
                                  const void* z, const float* delta_bias, void* out, float* x_ckpt, float* last_state,
                                  int batch, int dim, int seqlen, int dstate, int dt_rank, int io_dtype,
                                  long long z_bstride, long long xdbl_bstride, long long xdbl_tstride, int ckpt_step,
                                  int variant, void* stream);
int simamba_selective_scan_dt_bwd(const void* u, const void* xdbl, const void* wdt, const float* A, const float* D,
                                  const void* z, const float* delta_bias, const void* dout, const float* x_ckpt,
                                  void* du, void* ddelta, float* dA, float* dB, float* dC, float* dD, void* dz,
                                  float* ddelta_bias, int batch, int dim, int seqlen, int dstate, int dt_rank,
                                  int io_dtype, long long z_bstride, long long dz_bstride, long long xdbl_bstride,
                                  long long xdbl_tstride, void* stream);
/* ... and its deterministic form (flags / workspace as simamba_selective_scan_bwd_ex, ckpt_step _SEQ) */
int simamba_selective_scan_dt_bwd_ex(const void* u, const void* xdbl, const void* wdt, const float* A, const float* D,
                                     const void* z, const float* delta_bias, const void* dout, const float* x_ckpt,
                                     void* du, void* ddelta, float* dA, float* dB, float* dC, float* dD, void* dz,
                                     float* ddelta_bias, int batch, int dim, int seqlen, int dstate, int dt_rank,
                                     int io_dtype, long long z_bstride, long long dz_bstride, long long xdbl_bstride,
                                     long long xdbl_tstride, int flags, float* workspace, long long workspace_floats,
                                     void* stream);

/*
 * Fused x_proj -> dt_proj of the mixer on the matrix cores (the two skinny GEMMs between the conv and the scan
 * inside upstream's mamba_inner_fn, reached from models/block.py:72):
 *   xdbl[b, t, s]  = sum_d wx[s, d] * x[b, d, t]            (batch, seqlen, S) token-major, S = dt_rank + 2 * dstate
 *   delta[b, d, t] = sum_r wdt[d, r] * xdbl[b, t, r], r < R (batch, D, seqlen)
 *   x : (batch, D, seqlen), seqlen contiguous, batch stride x_bstride elements (0 => D * seqlen);
 *   wx : (S, D), wdt : (D, R), both in the I/O type.  SIMAMBA_F32: exact fp32 MFMA (v_mfma_f32_32x32x2_f32);
 *   SIMAMBA_BF16: v_mfma_f32_32x32x16_bf16 with fp32 accumulation and the roundings of the reference's autocast
 *   run (x_conv, x_dbl, delta each rounded once; delta formed from the rounded dt rows).
 *   D % 64 == 0, D * seqlen * 4 < 2^32 (one sample is one buffer descriptor), seqlen % 4 == 0 (bf16: % 8), S % 4 == 0, S <= 64,
 *   R % 4 == 0, 4 <= R <= 24, 16-byte aligned pointers; anything else returns SIMAMBA_E_SHAPE / _ALIGN (the host
 *   mirror then takes the two library GEMMs).
 *   delta == NULL: only xdbl (and xconv) are produced -- the delta product is left to simamba_selective_scan_dt_fwd.
 */
int simamba_xdt_proj_fwd(const void* x, const void* wx, const void* wdt, void* xdbl, void* delta,
                         int batch, int D, int seqlen, int S, int R, int io_dtype, long long x_bstride,
                         void* stream);
/* The same with the causal depthwise conv1d (width 4, bias cb or NULL, + SiLU) of the mixer applied to x on the way
 * in (causal_conv1d_fn inside the same mamba_inner_fn): xconv (batch, D, seqlen) receives silu(conv(x)) -- what the
 * scan and the backward read -- so conv, x_proj and dt_proj are one pass over the in_proj output's x half.
 * D <= 1024 (taps and bias are held in LDS). */
int simamba_conv_xdt_proj_fwd(const void* x, const float* cw, const float* cb, const void* wx, const void* wdt,
                              void* xconv, void* xdbl, void* delta, int batch, int D, int seqlen, int S, int R,
                              int io_dtype, long long x_bstride, void* stream);

/*
 * Token-sequence expansion along the last axis and its adjoint.  The reference's block stack sees L = 2 k G tokens
 * that are the same G patch tokens in 2 k orders (models/point_mamba.py:889-898, :982-989); the per-token head of the
 * first block (Add, LayerNorm, in_proj: models/block.py:56-60) is computed on the G distinct tokens and expanded:
 *   fwd: out[b, c, l] = in[b, c, idx[b, l]]              in (batch, channels, G), idx (batch, L) int32,
 *                                                        out (batch, channels, L) with batch stride out_bstride
 *   bwd: din[b, c, g] = sum_j dout[b, c, inv[b, g, j]]   inv (batch, G, R) int32: the R = L / G positions of token g
 *   G <= 256, L <= 2048, G % 4 == 0, L % 4 == 0, R <= 8; idx 16-byte aligned.  Deterministic (no atomics).
 */
int simamba_seq_gather_fwd(const void* in, const int* idx, void* out, int batch, int channels, int G, int L,
                           long long out_bstride, int io_dtype, void* stream);
int simamba_seq_gather_bwd(const void* dout, const int* inv, void* din, int batch, int channels, int G, int L,
                           int R, long long dout_bstride, int io_dtype, void* stream);

/*
 * Causal depthwise conv1d (+ optional SiLU).
 *   x, out, dout, dx : (batch, dim, seqlen) io_dtype
 *   w : (dim, width) fp32; bias : (dim) fp32 or NULL; dw, dbias fp32, zeroed then accumulated (float atomics:
 *   last-bit run-to-run jitter; the _ex form with SIMAMBA_BWD_DETERMINISTIC writes them whole, bitwise reproducible,
 *   from per-workgroup partials in `workspace`, contract as simamba_selective_scan_bwd_ex).
 *   out[b,d,t] = act(bias[d] + sum_k w[d,k] * x[b,d,t-(width-1)+k])
 *   x_bstride / dx_bstride: elements between batch samples of x / dx (0 => dim*seqlen).
 */
int simamba_causal_conv1d_fwd(const void* x, const float* w, const float* bias, void* out,
                              int batch, int dim, int seqlen, int width, int silu,
                              int io_dtype, long long x_bstride, void* stream);
int simamba_causal_conv1d_bwd(const void* x, const float* w, const float* bias,
                              const void* dout, void* dx, float* dw, float* dbias,
                              int batch, int dim, int seqlen, int width, int silu,
                              int io_dtype, long long x_bstride, long long dx_bstride, void* stream);
long long simamba_causal_conv1d_bwd_workspace_floats(int batch, int dim, int seqlen, int width, int flags);
int simamba_causal_conv1d_bwd_ex(const void* x, const float* w, const float* bias,
                                 const void* dout, void* dx, float* dw, float* dbias,
                                 int batch, int dim, int seqlen, int width, int silu,
                                 int io_dtype, long long x_bstride, long long dx_bstride, int flags,
                                 float* workspace, long long workspace_floats, void* stream);

/*
 * Fused (DropPath-scaled) residual add + LayerNorm: the "Add -> LayerNorm" half of the reference's
 * Block.forward (models/block.py:56-60) and the final norm of MixerModel (models/point_mamba.py:257-258).
 *   hidden        : (batch, rows_per_batch, dim) hidden_dtype
 *   residual      : same shape fp32, or NULL (first block: residual_out = hidden, not written when
 *                   residual_out is NULL)
 *   rowscale      : (batch) fp32 or NULL -- DropPath keep-mask / keep-prob per sample, applied to hidden
 *                   only when residual != NULL (the reference does not drop the first block's input)
 *   residual_out  : fp32 ; normed : out_dtype ; mean, rstd : (batch * rows_per_batch) fp32
 *   residual_out = hidden * rowscale + residual ;  normed = LayerNorm(residual_out; weight, bias, eps)
 * Backward: dresidual (fp32, gradient w.r.t. `residual`) = LN'(dnormed) + dresidual_out ;
 *   dhidden (hidden_dtype) = dresidual * rowscale ; either may be NULL (not both).
 *   dwb_partial : (simamba_add_layer_norm_grid(batch, rows_per_batch), 2, dim) fp32 -- per-workgroup partial
 *   sums of (dweight, dbias); the caller reduces over the first axis.
 * dim % 4 == 0, dim <= 2048.
 */
int simamba_add_layer_norm_grid(int batch, int rows_per_batch);
int simamba_add_layer_norm_fwd(const void* hidden, const float* residual, const float* rowscale,
                               const float* weight, const float* bias, float* residual_out,
                               void* normed, float* mean, float* rstd, int batch, int rows_per_batch,
                               int dim, float eps, int hidden_dtype, int out_dtype, void* stream);
int simamba_add_layer_norm_bwd(const void* dnormed, const float* dresidual_out,
                               const float* residual_out, const float* mean, const float* rstd,
                               const float* weight, const float* rowscale, float* dresidual,
                               void* dhidden, float* dwb_partial, int batch, int rows_per_batch,
                               int dim, int hidden_dtype, int out_dtype, void* stream);

/*
 * Norm flags of the *_ex forms of the add + norm entry points (0 = LayerNorm: the plain entry point, bit for bit).
 *   SIMAMBA_NORM_RMS: RMSNorm (mamba-ssm's RMSNorm, the reference's rms_norm=True: models/point_mamba.py:164, :227)
 *   in place of LayerNorm:  rstd = 1 / sqrt(mean(x^2) + eps), normed = x * rstd * weight.  No mean, no bias:
 *   bias / beta must be NULL (else SIMAMBA_E_BIAS); mean is neither read nor written and may be NULL.  Backward:
 *   dresidual = rstd * (g - x^ * mean(g * x^)) + dresidual_out with x^ = x * rstd, g = dnormed * weight; dwb_partial
 *   keeps its (grid, 2, dim) layout, row 0 of each partial = dweight, row 1 (dbias) unspecified (not written).
 *   Unknown flag bits: SIMAMBA_E_VARIANT.  Both flag checks precede every other check.
 */
#define SIMAMBA_NORM_RMS 1
int simamba_add_layer_norm_fwd_ex(const void* hidden, const float* residual, const float* rowscale,
                                  const float* weight, const float* bias, float* residual_out,
                                  void* normed, float* mean, float* rstd, int batch, int rows_per_batch,
                                  int dim, float eps, int hidden_dtype, int out_dtype, int flags, void* stream);
int simamba_add_layer_norm_bwd_ex(const void* dnormed, const float* dresidual_out,
                                  const float* residual_out, const float* mean, const float* rstd,
                                  const float* weight, const float* rowscale, float* dresidual,
                                  void* dhidden, float* dwb_partial, int batch, int rows_per_batch,
                                  int dim, int hidden_dtype, int out_dtype, int flags, void* stream);

/*
 * ... on compact batches.  `hidden` / `dhidden` hold hidden_batch <= batch samples and `normed` / `dnormed` hold
 * normed_batch <= batch samples, packed; everything else (residual, residual_out, dresidual_out, dresidual, mean,
 * rstd, rowscale) stays (batch, ...), and so do the grid and the layout of dwb_partial.
 *   hidden_slot : (batch) int32 on the device -- sample b's index inside hidden / dhidden, or -1: the sample has no
 *                 hidden rows.  Forward: residual_out = residual for it, hidden is not read (what a rowscale of 0
 *                 gives).  Backward: dhidden = rowscale * dresidual is written for the mapped samples only, at their
 *                 slot (zeros where rowscale is 0).  Needs residual and residual_out.
 *   normed_slot : (batch) int32 on the device -- sample b's index inside normed / dnormed, or -1: nobody needs the
 *                 sample's normed rows.  Forward: neither normed nor mean / rstd are written for it.  Backward: its
 *                 dresidual = dresidual_out (0 without one), it adds nothing to dwb_partial (what a zero dnormed
 *                 gives), and its residual_out, mean, rstd and dnormed are not read.
 * A NULL map says the tensor holds the whole batch and goes with a compact batch == batch (else SIMAMBA_E_NULLPTR);
 * with NULL maps these are simamba_add_layer_norm_fwd_ex / _bwd_ex bit for bit.  A compact batch outside [0, batch]:
 * SIMAMBA_E_SHAPE.  A compact batch of 0 is legal and its tensor may be NULL.  The maps live on the device and are not
 * read by the host: the kernels treat a slot outside [-1, compact batch) as -1, and every slot in [0, compact batch)
 * of dhidden that is read afterwards has to be some sample's.  simamba_add_layer_norm_check_slots checks a map that is
 * still on the HOST (no stream): SIMAMBA_E_SHAPE for an entry outside [-1, compact_batch), a slot taken twice or a
 * compact batch outside [0, batch], SIMAMBA_E_NULLPTR without a map.
 */
int simamba_add_layer_norm_check_slots(const int* slots_host, int batch, int compact_batch);
int simamba_add_layer_norm_fwd_slots(const void* hidden, const float* residual, const float* rowscale,
                                     const float* weight, const float* bias, float* residual_out,
                                     void* normed, float* mean, float* rstd, const int* hidden_slot,
                                     int hidden_batch, const int* normed_slot, int normed_batch, int batch,
                                     int rows_per_batch, int dim, float eps, int hidden_dtype, int out_dtype,
                                     int flags, void* stream);
int simamba_add_layer_norm_bwd_slots(const void* dnormed, const float* dresidual_out,
                                     const float* residual_out, const float* mean, const float* rstd,
                                     const float* weight, const float* rowscale, float* dresidual,
                                     void* dhidden, float* dwb_partial, const int* hidden_slot,
                                     int hidden_batch, const int* normed_slot, int normed_batch, int batch,
                                     int rows_per_batch, int dim, int hidden_dtype, int out_dtype, int flags,
                                     void* stream);

/*
 * out_proj -> (+ DropPath-scaled residual) -> LayerNorm in one kernel on the matrix cores, bf16 operands: the mixer's
 * out_proj (upstream mamba_inner_fn, models/block.py:72) fused with the Add -> LayerNorm that opens the next block
 * (models/block.py:56-58) or closes the stack (models/point_mamba.py:257-258).  The out_proj result is rounded to bf16
 * (the rounding the reference's autocast GEMM output has) and never written:
 *   y : (batch, K, L) bf16, L contiguous ; w : (C, K) bf16 ; residual : (batch, L, C) fp32 or NULL ;
 *   rowscale : (batch) fp32 or NULL (applied to the out_proj result when residual != NULL) ; gamma, beta : (C) fp32 ;
 *   residual_out : (batch, L, C) fp32 = bf16(y^T w^T) * rowscale + residual ; normed : out_dtype = LayerNorm(residual_out) ;
 *   mean, rstd : (batch * L) fp32 for simamba_add_layer_norm_bwd.
 * C % 128 == 0, C <= 384, K % 64 == 0, L % 8 == 0, K * L * 2 < 2^32, 16-byte aligned pointers.
 */
int simamba_out_proj_add_ln_fwd(const void* y, const void* w, const float* residual, const float* rowscale,
                                const float* gamma, const float* beta, float* residual_out, void* normed, float* mean,
                                float* rstd, int batch, int K, int L, int C, float eps, int out_dtype, void* stream);
/* ... with the norm flags above (SIMAMBA_NORM_RMS: beta NULL, mean may be NULL; the backward is
 * simamba_add_layer_norm_bwd_ex with the same flags) */
int simamba_out_proj_add_ln_fwd_ex(const void* y, const void* w, const float* residual, const float* rowscale,
                                   const float* gamma, const float* beta, float* residual_out, void* normed,
                                   float* mean, float* rstd, int batch, int K, int L, int C, float eps, int out_dtype,
                                   int flags, void* stream);

/*
 * in_proj of the mixer on the matrix cores (the first product of upstream's Mamba.forward, reached from
 * models/block.py:72):  xz[b, j, t] = sum_c w[j, c] * x[b, t, c].  Also the shape of out_proj's input gradient.
 *   x : (batch, L, C) io_dtype, token-major (the LayerNorm output) ; w : (M, C) io_dtype ; xz : (batch, M, L) io_dtype,
 *   L contiguous (the layout the conv / scan kernels stream).  fp32: exact fp32 MFMA (an fmaf chain); bf16: fp32
 *   accumulation, one rounding to bf16.
 * C % 64 == 0, C <= 384, M % 32 == 0, L % 8 == 0 (fp32: L % 4 == 0), 16-byte aligned pointers.  A workgroup owns 256
 * (fp32: 128) tokens of one sample: grids of fewer than ~200 workgroups leave CUs idle and are better served by the
 * library GEMM.
 */
int simamba_in_proj_fwd(const void* x, const void* w, void* xz, int batch, int L, int C, int M, int io_dtype,
                        void* stream);

/*
 * Patch-encoder streaming ops (reference models/point_mamba.py:46-73, Encoder: Conv1d - BatchNorm1d - ReLU -
 * Conv1d, max over the n points of a patch; the 1x1 convolutions are GEMMs on token-major (rows, C) tensors).
 *
 * simamba_bn_relu_fwd: y = relu(BatchNorm(x + g)) with g[r / group][c] an optional per-group additive term
 * (gterm == NULL: none).  training != 0: batch statistics over all rows (biased variance for the
 * normalisation, unbiased for running_var; running_* updated with `momentum` when non-NULL), written to
 * mean / invstd (C) for the backward; training == 0: running statistics.  weight / bias may be NULL (1 / 0).
 *   x, y : (rows, C) io_dtype with row stride ld elements (0 = C; a channel slice of a wider tensor is
 *   processed in place: C <= 1024 per call, wider layers are done slice by slice) ; gterm : (rows / group, C)
 *   fp32 ; partial : (simamba_bn_relu_grid(rows), 2, C) fp32 scratch.  C % 4 == 0, ld % 4 == 0,
 *   rows % group == 0.
 * simamba_bn_relu_bwd: dx (rows, C) io_dtype (same ld), dgterm (rows / dgroup, C) fp32 or NULL (= sum of dx over
 *   runs of dgroup rows; 256 % dgroup == 0 -- for group > 256 the caller sums group / 256 consecutive rows of
 *   it), dweight, dbias (C) fp32 ; same partial scratch.
 * simamba_group_max_fwd/bwd: out[g][c] = max_r x[g][r][c] over r < n (first maximum; NaN propagates), idx the
 *   arg max as uint8 (n <= 256); backward routes dout to that row and writes zeros elsewhere (one pass).
 *
 * The same passes as separate stages, for batch statistics taken over the rows of several ranks (nn.SyncBatchNorm):
 * the caller puts one collective between them each way.  Shapes, ld, gterm / group, dgterm / dgroup and the order of
 * the argument checks (dtype, empty, shape, null pointers) are those of the two calls above.
 * simamba_bn_stats_local: pass 1 and its fp64 finalize over this rank's rows.  stats : (3, C) fp64 with row stride
 *   stats_ld (0 = C; a channel slice writes into the block of the whole layer): row 0 the row count, row 1 the mean,
 *   row 2 M2 = sum (x + g - mean)^2 -- free of the rank's own shift, so blocks of different ranks merge.  Running
 *   statistics are not touched.
 * simamba_bn_stats_merge: stats : (world, 3, C) fp64 contiguous, the all-gather of the ranks' blocks (any C >= 1, the
 *   whole layer in one call).  Merged in fp64 in rank order 0 .. world-1 with the pairwise update n = na + nb,
 *   d = mb - ma, mean = ma + d nb / n, M2 = M2a + M2b + d^2 na nb / n: the same bits on every rank.  Writes mean,
 *   invstd = 1 / sqrt(M2 / n + eps) (C) fp32, count (1) fp64 = n, and updates running_mean / running_var (non-NULL)
 *   with `momentum`, running_var from the unbiased variance M2 / (n - 1) of the total count.
 * simamba_bn_relu_apply: pass 2, y = relu((x + g - mean) * invstd * w + b), with the caller's mean / invstd.
 * simamba_bn_relu_bwd_sums: the backward's pass 1 and its finalize: dbias = sum dy*mask and
 *   dweight = sum dy*mask*xhat over THIS rank's rows, with the global mean / invstd.
 * simamba_bn_relu_bwd_dx: the backward's pass 2 with sum_dweight / sum_dbias (C) fp32 summed over all ranks and
 *   count (1) fp64, the row count of all ranks, read on the device (the buffer simamba_bn_stats_merge wrote).
 */
int simamba_bn_relu_grid(long long rows);
int simamba_bn_relu_fwd(const void* x, const float* gterm, int group, const float* weight, const float* bias,
                        float* running_mean, float* running_var, float momentum, float eps, int training,
                        void* y, float* mean, float* invstd, float* partial, long long rows, int C,
                        long long ld, int io_dtype, void* stream);
int simamba_bn_relu_bwd(const void* dy, const void* x, const float* gterm, int group, const float* weight,
                        const float* bias, const float* mean, const float* invstd, void* dx, float* dgterm,
                        int dgroup, float* dweight, float* dbias, float* partial, long long rows, int C,
                        long long ld, int io_dtype, int training, void* stream);
int simamba_bn_stats_local(const void* x, const float* gterm, int group, double* stats, long long stats_ld,
                           float* partial, long long rows, int C, long long ld, int io_dtype, void* stream);
int simamba_bn_stats_merge(const double* stats, int world, float* running_mean, float* running_var, float momentum,
                           float eps, float* mean, float* invstd, double* count, int C, void* stream);
int simamba_bn_relu_apply(const void* x, const float* gterm, int group, const float* weight, const float* bias,
                          const float* mean, const float* invstd, void* y, long long rows, int C, long long ld,
                          int io_dtype, void* stream);
int simamba_bn_relu_bwd_sums(const void* dy, const void* x, const float* gterm, int group, const float* weight,
                             const float* bias, const float* mean, const float* invstd, float* dweight,
                             float* dbias, float* partial, long long rows, int C, long long ld, int io_dtype,
                             void* stream);
int simamba_bn_relu_bwd_dx(const void* dy, const void* x, const float* gterm, int group, const float* weight,
                           const float* bias, const float* mean, const float* invstd, const float* sum_dweight,
                           const float* sum_dbias, const double* count, void* dx, float* dgterm, int dgroup,
                           long long rows, int C, long long ld, int io_dtype, void* stream);
int simamba_group_max_fwd(const void* x, void* out, unsigned char* idx, long long groups, int n, int C,
                          int io_dtype, void* stream);
int simamba_group_max_bwd(const void* dout, const unsigned char* idx, void* dx, long long groups, int n, int C,
                          int io_dtype, void* stream);

/*
 * Backward of y = max over the n rows of a patch of (x W^T + b), without the dense (groups * n, c_out) gradient between
 * the max and the product (csrc/encoder_sparse.hip).  idx (groups, c_out) uint8 is what simamba_group_max_fwd left;
 * an entry >= n contributes nothing.  fp32 arithmetic, no atomics, every sum in a fixed order: the same bits on every
 * call.
 *   dout : (groups, c_out) io_dtype ; weight : (c_out, c_in) io_dtype ; x, dx : (groups * n, c_in) io_dtype, all
 *   contiguous and 16-byte aligned (else SIMAMBA_E_ALIGN).  1 <= n <= 32, c_in % 64 == 0, c_out % 4 == 0,
 *   c_out <= 384 (else SIMAMBA_E_SHAPE).  Checks in the order dtype, empty, shape, null pointers, alignment.
 * simamba_max_linear_bwd_dx: dx[g n + r][:] = sum over {c : idx[g][c] == r} of dout[g][c] * weight[c][:], ascending c;
 *   every row is written once, rows no channel chose as zeros.
 * simamba_max_linear_bwd_dw: dw[c][:] = sum over g of dout[g][c] * x[g n + idx[g][c]][:] in fp32, (c_out, c_in);
 *   partial: simamba_max_linear_bwd_slabs(groups, c_in) * c_out * c_in floats of scratch (per-slab sums, added in slab
 *   order).
 */
int simamba_max_linear_bwd_slabs(long long groups, int c_in);
int simamba_max_linear_bwd_dx(const void* dout, const unsigned char* idx, const void* weight, void* dx,
                              long long groups, int n, int c_in, int c_out, int io_dtype, void* stream);
int simamba_max_linear_bwd_dw(const void* dout, const unsigned char* idx, const void* x, float* dw, float* partial,
                              long long groups, int n, int c_in, int c_out, int io_dtype, void* stream);

/*
 * Feature propagation of the part-segmentation head (reference part_segmentation/models/pointnet2_utils.py:262-305,
 * PointNetFeaturePropagation.forward): for every query point the three nearest of the sample's S centres
 * (squared distance in the reference's expanded form, ties to the lower index), weights 1/(d + 1e-8) normalised
 * to sum 1, and the weighted sum of the three centres' feature rows.
 *   xyz1 : (batch, N, 3) fp32 query points ; xyz2 : (batch, S, 3) fp32 centres ; idx : (batch, N, 3) int32 ;
 *   weight : (batch, N, 3) fp32 ; feats : (batch, S, C) io_dtype ; out : (batch, N, C) io_dtype ;
 *   dfeats : (batch, S, C) fp32, every element written (deterministic gather, no atomics).  C % 4 == 0, S <= 8192,
 *   N <= 8192 for the backward.
 */
int simamba_three_nn(const float* xyz1, const float* xyz2, int* idx, float* weight, int batch, int N, int S,
                     void* stream);
int simamba_three_interpolate_fwd(const void* feats, const int* idx, const float* weight, void* out, int batch,
                                  int N, int S, int C, int io_dtype, void* stream);
int simamba_three_interpolate_bwd(const void* dout, const int* idx, const float* weight, float* dfeats, int batch,
                                  int N, int S, int C, int io_dtype, void* stream);

/*
 * Gather-sum-scatter over the rows of a sequence: the per-layer cross-merge of the SAST orderings (reference
 * models/point_mamba.py:350-370 cross_merg and :394-409, the model option add_after_layer) in one pass, and its adjoint.
 *   x, y        : (batch, L, C) io_dtype, contiguous; y must not alias x.  Every row of y named by scatter_idx is
 *                 written, no other.
 *   gather_idx  : (batch, M, G) int32, rows of x ; scatter_idx : (batch, M, G) int32, rows of y.
 * For every (b, g), with H = M / 2, gi_m = gather_idx[b, m, g] and si_m = scatter_idx[b, m, g]:
 *   s = ((x[b, gi_0] + x[b, gi_H]) + (x[b, gi_1] + x[b, gi_{H+1}])) + ... + (x[b, gi_{H-1}] + x[b, gi_{M-1}])
 *   y[b, si_m] = s for m = 0 .. M-1
 * in fp32, in exactly that order of additions, rounded once to io_dtype.  No atomics: the same bits every time.  With
 * maps that are bijections of [0, L) per sample the adjoint is the same call with the two maps swapped.
 * M even, 2 <= M <= 16, L == M * G, C % 4 == 0, batch <= 65535 (else SIMAMBA_E_SHAPE); x and y aligned to one lane's
 * four elements (else SIMAMBA_E_ALIGN).  Checks in the order dtype, empty (batch == 0: SIMAMBA_OK, nothing read),
 * shape, null pointers, alignment; all precede the launch.  The index VALUES are the caller's contract (0 <= value < L):
 * they are not validated on the device, and a value outside that range reads or writes outside the tensors.
 * Still ABI version 9: a symbol added, none changed.
 */
int simamba_gather_sum_scatter(const void* x, const int* gather_idx, const int* scatter_idx, void* y, int batch, int L,
                               int G, int M, int C, int io_dtype, void* stream);

/*
 * Chamfer distance of the MAE pre-training loss (reference models/point_mamba.py:2950, :3203:
 * pytorch3d.loss.chamfer_distance(pred, gt, batch_reduction=None) -- squared L2 to the nearest neighbour, mean over
 * each set's points, both directions summed; one value per pair of sets).
 *   pred : (pairs, n, 3) fp32 ; gt : (pairs, m, 3) fp32 ; dist : (pairs) fp32 ; idx1 : (pairs, n) uint8 nearest gt
 *   of every prediction ; idx2 : (pairs, m) uint8 nearest prediction of every gt point ; n, m <= 64.
 * Backward: dpred (pairs, n, 3) fp32 from ddist (pairs) (gt carries no gradient).
 */
int simamba_chamfer_fwd(const float* pred, const float* gt, float* dist, unsigned char* idx1, unsigned char* idx2,
                        long long pairs, int n, int m, void* stream);
int simamba_chamfer_bwd(const float* pred, const float* gt, const float* ddist, const unsigned char* idx1,
                        const unsigned char* idx2, float* dpred, long long pairs, int n, int m, void* stream);

/*
 * The same distance between whole clouds, with gradients for both sets (csrc/chamfer_large.hip): tiled kernels,
 * 1 <= n, m <= 8192 points per set, any number of pairs (pairs * (ceil(n / 256) + ceil(m / 256)) < 2^31).
 *   x : (pairs, n, 3) fp32 ; y : (pairs, m, 3) fp32 ; dist : (pairs) fp32 ;
 *   idx1 : (pairs, n) int32 nearest y of every x ; idx2 : (pairs, m) int32 nearest x of every y ;
 *   d1 : (pairs, n) fp32, d2 : (pairs, m) fp32 : the squared distances to those neighbours (direct differences,
 *   dx*dx + dy*dy + dz*dz; strict `<` in ascending index, so the lowest index wins a tie) ;
 *   dist[p] = mean_i d1[p][i] + mean_j d2[p][j], fp64 partial sums in a fixed order.  All outputs are written by every
 *   call; no workspace.  NaN / inf do not propagate: the search starts from 3.0e38 with a strict `<` (as in the
 *   small kernels), so such a query reports distance 3.0e38 and index 0.
 * Backward, from ddist (pairs) and the indices the forward left:
 *   dx[i] = ddist * ( 2/n (x_i - y[idx1[i]]) + 2/m sum over {j : idx2[j] == i} of (x_i - y_j) ), ascending j,
 *   dy symmetric.  dx (pairs, n, 3) or dy (pairs, m, 3) may be NULL: that gradient is skipped and nothing is written
 *   for it.  No atomics in either call: the same bits every time.
 * Checks in the order shape (SIMAMBA_E_SHAPE), empty (pairs == 0: SIMAMBA_OK, nothing read), null pointers.
 * The _ex forms take `queries`, the query points a thread keeps in registers: 0 = the library's choice (what the plain
 * forms pass: the largest of 4, 2, 1 that both sets fill and that leaves 512 workgroups), 1, 2 or 4 = that kernel
 * (parity tests: the outputs do not depend on it, bit for bit); anything else SIMAMBA_E_VARIANT, checked first.
 * Still ABI version 9: symbols added, none changed.
 */
int simamba_chamfer_large_fwd(const float* x, const float* y, float* dist, int* idx1, int* idx2, float* d1, float* d2,
                              long long pairs, int n, int m, void* stream);
int simamba_chamfer_large_bwd(const float* x, const float* y, const float* ddist, const int* idx1, const int* idx2,
                              float* dx, float* dy, long long pairs, int n, int m, void* stream);
int simamba_chamfer_large_fwd_ex(const float* x, const float* y, float* dist, int* idx1, int* idx2, float* d1,
                                 float* d2, long long pairs, int n, int m, int queries, void* stream);
int simamba_chamfer_large_bwd_ex(const float* x, const float* y, const float* ddist, const int* idx1, const int* idx2,
                                 float* dx, float* dy, long long pairs, int n, int m, int queries, void* stream);
/*
 * The same kernels for ragged batches (sets padded to a common n, m) and the rest of pytorch3d's arguments but normals.
 *   xlen, ylen : (pairs) int32, device, or NULL (= n, m everywhere): pair p is the first xlen[p] points of x[p] against
 *                the first ylen[p] of y[p]; nothing at or behind a length is read.  The kernels clamp the values to
 *                [1, n] and [1, m]; the library never reads them on the host.  Every pair's outputs are what the pair
 *                returns alone at its true lengths, bit for bit; rows behind a length are written as 0 (index 0).
 *   norm       : 2 = squared L2 as above ; 1 = |dx| + |dy| + |dz|, gradient sign(a - b) per coordinate, sign(0) = 0.
 *   reduction  : 0 mean: dist[p] = sum_i d1[p][i] / xlen[p] + sum_j d2[p][j] / ylen[p] ; 1 sum: no division ;
 *                2 none: dist is not written and may be NULL, and the backward takes per-point upstream gradients
 *                dd1 (pairs, n), dd2 (pairs, m) in place of ddist (pairs); whichever of the two is unused may be NULL.
 *   flags      : bit 0 = one-way (x against y only): idx2, d2, dd2 are not touched and may be NULL, dist has the x term
 *                only, dx has only the own-nearest term and dy only the reverse matches,
 *                dy[j] = -k sum over {i : idx1[i] == j} of (x_i - y_j), ascending i.
 *   queries    : as in the _ex forms.
 * dx or dy may be NULL as above; rows behind a length get exactly 0.  No atomics: the same bits every time.
 * Checks in the order variant (queries, norm, reduction, flags: SIMAMBA_E_VARIANT), shape, empty (pairs == 0:
 * SIMAMBA_OK, nothing read), null pointers.  With xlen = ylen = NULL, norm 2, reduction 0 and flags 0 these are the _ex
 * forms (which are that call).  Still ABI version 9: symbols added, none changed.
 */
int simamba_chamfer_ragged_fwd(const float* x, const float* y, const int* xlen, const int* ylen, float* dist,
                               int* idx1, int* idx2, float* d1, float* d2, long long pairs, int n, int m, int norm,
                               int reduction, int flags, int queries, void* stream);
int simamba_chamfer_ragged_bwd(const float* x, const float* y, const int* xlen, const int* ylen, const float* ddist,
                               const float* dd1, const float* dd2, const int* idx1, const int* idx2, float* dx,
                               float* dy, long long pairs, int n, int m, int norm, int reduction, int flags,
                               int queries, void* stream);

/*
 * Earth mover's distance between pairs of equal-sized point sets (csrc/emd.hip): the cost of the cheapest one-to-one
 * matching under squared Euclidean distance, c_ij = (dx*dx + dy*dy) + dz*dz, by the forward auction with Jacobi rounds
 * and epsilon-scaling.  The x points bid, the y points are the objects; every cost is formed on the fly from LDS.
 *   x, y      : (pairs, n, 3) fp32, contiguous ; 1 <= n <= 1024 ; pairs >= 1.
 *   assign    : (pairs, n) int32, assign[p][i] = the y point matched to x[p][i]; always a permutation of 0 .. n-1.
 *   dist      : (pairs) fp32 = mean_i |x_i - y_assign[i]|^2.
 *   rounds    : (pairs) int32, bidding rounds run, over all phases.
 *   converged : (pairs) uint8, 1 when the last phase ended with every bidder assigned: then the matching's total cost
 *               is within n * eps_final of the optimum.  0: the round cap was reached first; the bidders still
 *               unassigned took the objects still free, both in index order, and nothing is promised about the cost.
 *   eps       : eps_final, absolute, in cost units; 0 = 2^-14 * cmax of each pair, cmax the pair's largest cost (1e-30
 *               where cmax is 0).  Phases run with cmax/2, cmax/8, ... down to eps_final; prices carry over.
 *   max_rounds: the cap on `rounds` per pair; every loop of the kernel is bounded by it, whatever the input.
 * A winning bid raises the price to max(bid, nextafter(old price)), so a round always makes progress, also with eps
 * below the price's ulp.  Equal bids on one object go to the lowest bidder index: no result depends on timing, the same
 * bits every time.  Non-finite coordinates: no index is ever derived from a float, the kernel ends at the cap at the
 * latest and assign is still a permutation; dist is then whatever that matching costs (inf or NaN), converged
 * usually 0.  n <= 64: one wave per pair, four pairs per workgroup; above: one workgroup per pair.  No workspace, no
 * global atomics, no allocation or synchronisation.
 * Checks: SIMAMBA_E_SHAPE (n outside [1, 1024], pairs < 1, max_rounds < 1, eps negative or NaN), then null pointers.
 * Still ABI version 9: a symbol added, none changed.
 */
int simamba_emd_fwd(const float* x, const float* y, int* assign, float* dist, int* rounds, unsigned char* converged,
                    long long pairs, int n, float eps, int max_rounds, void* stream);

/*
 * Debiased Sinkhorn divergence between pairs of point sets of unequal size (csrc/sinkhorn.hip), the entropic transport
 * distance beside simamba_emd_fwd: uniform masses a = 1/nx, b = 1/ny, costs c_ij = (dx*dx + dy*dy) + dz*dz formed on
 * the fly from LDS.  Per pair, diam2 = the squared diagonal of the bounding box of its nx + ny points (at least 1e-30);
 * S = ceil(log2(1 / eps_rel)) scaling steps at eps_t = diam2 * 2^-t, t = 0 .. S-1, then `iters` steps at
 * eps_fin = diam2 * eps_rel; one step, from g = 0:
 *   f_i <- -eps log sum_j b_j exp((g_j - c_ij) / eps), then g_j <- -eps log sum_i a_i exp((f_i - c_ij) / eps).
 * OT(x, y) = sum_i a_i f_i + sum_j b_j g_j at the final iterates; (x, x) and (y, y) run the same schedule with the
 * pair's diam2.  The schedule is known on the host; no device value is read back.
 *   x, y       : (pairs, n, 3), (pairs, m, 3) fp32, contiguous ; 1 <= n, m <= 8192 ; pairs >= 1 and
 *                pairs * 2 * (ceil(n / 64) + ceil(m / 64)) < 2^31 (the largest grid).
 *   xlen, ylen : (pairs) int32, device, or NULL (= n, m everywhere), as in simamba_chamfer_ragged_fwd: clamped to
 *                [1, n], [1, m] by the kernels, nothing at or behind a length is read (the padding may hold NaN),
 *                potentials and gradients behind a length are written as 0, and every pair's outputs are bit for bit
 *                what it returns alone at its true lengths.
 *   eps_rel    : 0 < eps_rel <= 1 ; iters >= 0 ; 1 <= S + iters <= 4096.
 *   flags      : bit 0 = SIMAMBA_SINKHORN_DEBIAS: div = OT(x, y) - OT(x, x) / 2 - OT(y, y) / 2; without it div = OT(x, y),
 *                g_xx, g_yy, f_yy are not touched and may be NULL.
 *   div, ot_xy : (pairs) fp32.  fp64 partial sums in a fixed order.
 *   merr       : (pairs) fp32 or NULL (then not computed): sum_i a_i |1 - exp((f_i - f_i+) / eps_fin)|, f+ one further
 *                f-update of (x, y) that is not stored: the row-marginal error of the plan after the last step.
 *   f_xy, g_xx : (pairs, n) ; g_xy, g_yy, f_yy : (pairs, m) fp32: the potentials after the last step.
 * Backward, the potentials held fixed (exact at convergence), from ddiv (pairs):
 *   dx_i = ddiv a_i 2 ( sum_j pi_xy(j|i) (x_i - y_j) - sum_k pi_xx(k|i) (x_i - x_k) ),
 *   pi_xy(j|i) = softmax_j((g_xy_j - c_ij) / eps_fin), pi_xx the same from g_xx; dy_j likewise from f_xy and f_yy (the
 *   potentials that are g_xy and g_xx bit for bit when y is x, so that the divergence of a set from itself is 0.0 and
 *   both its gradients are exactly 0).  Without the flag the second sum is absent.  dx (pairs, n, 3) or dy
 *   (pairs, m, 3) may be NULL: that gradient is skipped, and the potentials only it reads may be NULL too.
 *   workspace  : device memory, 16-byte aligned (else SIMAMBA_E_ALIGN), at least simamba_sinkhorn_workspace_bytes()
 *                bytes (else, or NULL, SIMAMBA_E_WORKSPACE): diam2, the per-row marginal errors and f_xx; the backward
 *                needs 4 * pairs bytes of it.  The query answers 0 for arguments the calls refuse.
 * A NaN coordinate inside a length makes that pair's outputs NaN and no other's; every loop has a host-known trip
 * count.  No atomics: the same bits every call.
 * Checks in the order flags (SIMAMBA_E_VARIANT), shape (SIMAMBA_E_SHAPE: sizes, pairs, eps_rel, iters), null pointers,
 * workspace; all before any launch.  Still ABI version 9: symbols added, none changed.
 */
#define SIMAMBA_SINKHORN_DEBIAS 1
size_t simamba_sinkhorn_workspace_bytes(long long pairs, int n, int m, int flags);
int simamba_sinkhorn_fwd(const float* x, const float* y, const int* xlen, const int* ylen, float* div, float* ot_xy,
                         float* merr, float* f_xy, float* g_xy, float* g_xx, float* g_yy, float* f_yy, long long pairs,
                         int n, int m, float eps_rel, int iters, int flags, void* workspace, size_t workspace_bytes,
                         void* stream);
int simamba_sinkhorn_bwd(const float* x, const float* y, const int* xlen, const int* ylen, const float* ddiv,
                         const float* f_xy, const float* g_xy, const float* g_xx, const float* f_yy, float* dx,
                         float* dy, long long pairs, int n, int m, float eps_rel, int flags, void* workspace,
                         size_t workspace_bytes, void* stream);

/*
 * Part-segmentation scoring (csrc/part_metrics.hip; the reference's evaluation loop, part_segmentation/main.py:269-334):
 * the argmax of every point's scores restricted to the labels of its shape's category, and the counts that accuracy,
 * class-average accuracy and the two mean IoUs are made of.  One workgroup per shape, integers until the last division.
 *   scores     : (batch, n, c) SIMAMBA_F32 or SIMAMBA_BF16, contiguous; log-probabilities or logits, only their order
 *                matters.  1 <= c <= 256 ; n >= 1 ; 1 <= batch < 2^31.
 *   target     : (batch, n) int64, the true label of every point.
 *   part_first,
 *   part_count : (batch) int32 each, device: the label range [first, first + count) of the shape's category,
 *                1 <= count <= 16, first + count <= c.  The kernel clamps count into [1, min(16, c)] and first into
 *                [0, c - count]; the library never reads them on the host.
 *   lengths    : (batch) int64, device, or NULL (= n everywhere), as in simamba_farthest_point_sample_ex: shape b is
 *                its first lengths[b] points, clamped to [1, n] by the kernel; neither scores nor target are read at or
 *                behind a length (the padding may hold NaN and any label).
 *   pred       : (batch, n) int64 or NULL (then not written): first + argmax(scores[b][i][first .. first + count)), -1
 *                behind a length.  The FIRST maximum; a NaN counts as greater than every number and the first NaN wins
 *                (numpy's argmax); +inf and -inf order as numbers.
 *   inter, uni : (batch, 16) int32: for part k of the shape's category, l = first + k, the points with target == l and
 *                pred == l, and those with target == l or pred == l.  Columns >= count are written as 0.
 *   shape_iou  : (batch) fp64 = the mean over k < count of inter / uni, a part with uni == 0 (absent and unpredicted)
 *                contributing 1.0: divided, added in part order and divided by count in double.
 *   correct    : (batch) int32, the points with pred == target.
 *   seen_class,
 *   correct_class : (c) int64 each, ACCUMULATED INTO (the caller zeroes them): over all points, target == l, and
 *                pred == l and target == l.  The only sums across workgroups: 64-bit integer atomics.
 * A target outside the category's range matches no prediction but is still counted in seen_class; a target outside
 * [0, c) is counted nowhere and indexes nothing.  No float or double atomic, no workspace, no allocation or
 * synchronisation: the same bits every call.
 * Checks in the order shape (SIMAMBA_E_SHAPE: batch, n, c), dtype (SIMAMBA_E_DTYPE), null pointers (all but lengths
 * and pred are required); all before any launch.  Still ABI version 9: a symbol added, none changed.
 */
int simamba_part_seg_eval(const void* scores, const long long* target, const int* part_first, const int* part_count,
                          const long long* lengths, long long* pred, int* inter, int* uni, double* shape_iou,
                          int* correct, long long* seen_class, long long* correct_class, long long batch, int n, int c,
                          int io_dtype, void* stream);

/*
 * Linear one-vs-one C-SVC (csrc/svm.hip): the reference's per-epoch pre-training score, tools/runner_pretrain.py:66-77,
 * scikit-learn's SVC(C=0.01, kernel='linear'), i.e. libsvm.  THIS FAMILY IS FLOAT64 -- the one exception to "all state
 * fp32" above: the solver's gradient sums are of size n_SV * C * |K| against a tolerance of 1e-3.
 *
 * simamba_svm_ovo_fit: one workgroup per class pair (a, b), a < b, pairs in libsvm's order (0,1), (0,2), ...
 * (nc-2, nc-1), P = nc (nc - 1) / 2 of them.  A pair's problem is class a's samples (y = +1) followed by class b's
 * (y = -1); it solves  min 1/2 a'Qa - e'a,  0 <= a <= C,  y'a = 0,  Q = yy' o gram  by SMO with libsvm's second-order
 * working-set rule (curvature floor 1e-12), libsvm's clipped update, libsvm's stopping rule m(a) - M(a) < tol and
 * libsvm's rho (the mean of yG over the free a; with none free, the midpoint of the two bounds).
 *   gram        : (n, n) fp64, row-major, the training Gram matrix x x'.      2 <= n <= 16384.
 *   x           : (n, d) fp32 feature rows (read once per pair, for w).       1 <= d <= 4096.
 *   order       : (n) int32, device: the sample indices grouped by class, input order kept inside a class.  Entries are
 *                 clamped into [0, n) by the kernel.
 *   class_start : (nc + 1) int32, a HOST array read during the call: class k is order[class_start[k] ..
 *                 class_start[k + 1]).  class_start[0] == 0, class_start[nc] == n, no class empty, and no two classes
 *                 together above 4096 samples (a pair lives in LDS); 2 <= nc <= 64.
 *   alpha       : (nc - 1) * n fp64: the pairs' alpha back to back in pair order, each in the pair's sample order.  The
 *                 kernel derives every pair's offset from class_start itself; 0 <= alpha <= C holds exactly.
 *   w           : (P, d) fp64 = sum_k alpha_k y_k x_k, accumulated in fp64 in sample order.
 *   rho         : (P) fp64; the pair's decision value of a row z is w . z - rho, positive for class a.
 *   n_iter      : (P) int32, updates made.
 *   converged   : (P) uint8, 1 when the stopping rule was met; 0: the cap was reached first (alpha is still feasible),
 *                 or gram holds a NaN.
 *   c_tol       : a HOST array of two fp64 read during the call, {C, tol}, both > 0 (the ABI passes no double by
 *                 value).
 *   max_iter >= 1, max_iter_per_sample >= 0: a pair of n_p samples makes at most
 *                 max_iter + max_iter_per_sample * n_p updates (capped at 2^31 - 1); every loop of the kernel is bounded
 *                 by it, whatever the input, and all waves leave in the same iteration.
 * No atomics, ties to the lower position, every reduction in a fixed order: the same bits every call.
 * Checks in the order shape (SIMAMBA_E_SHAPE: nc, n, d, the iteration caps, then -- each when its host array is not
 * NULL -- C or tol <= 0 or NaN, and class_start's ends, an empty class, a pair above 4096), null pointers (all
 * required); all before any launch.
 *
 * simamba_svm_ovo_vote: libsvm's svm_predict_values on decision values, one wave per row.
 *   dec     : (m, P) fp64.  dec > 0 is a vote for a, anything else (exactly 0 and NaN too) for b; the class with the
 *             most votes wins, the lowest class index on a tie.                 1 <= m < 2^31 ; 2 <= nc <= 64.
 *   pred    : (m) int32, the winning class index.
 *   labels  : (m) int64 class indices, or NULL; with labels, the rows with pred == labels are ADDED to
 *   matches : (1) int64 (the caller zeroes it; one 64-bit integer atomic per matching row).  Required with labels.
 * Checks: SIMAMBA_E_SHAPE (nc, m), then null pointers.  Still ABI version 9: symbols added, none changed.
 */
int simamba_svm_ovo_fit(const double* gram, const float* x, const int* order, const int* class_start,
                        const double* c_tol, double* alpha, double* w, double* rho, int* n_iter,
                        unsigned char* converged, int n, int d, int nc, int max_iter, int max_iter_per_sample,
                        void* stream);
int simamba_svm_ovo_vote(const double* dec, const long long* labels, int* pred, long long* matches, long long m, int nc,
                         void* stream);

/*
 * Exact t-SNE in two dimensions (csrc/tsne.hip): the reference's map of the classifier's pooled features,
 * tools/runner_finetune.py:605-612, scikit-learn's TSNE with its schedule and its stop rule.  Storage is fp32; the sums
 * of the perplexity search, Z, the squared gradient norm and KL are fp64.  2 <= n <= 16384 throughout.
 *
 * simamba_tsne_calibrate: one workgroup per row i of d2, the (n, n) fp32 squared distances.  It finds beta_i with the
 * entropy of p_{j|i} ~ exp(-beta_i d2_ij), j != i, equal to log(perplexity): scikit-learn's search (start at 1, double
 * or halve until bracketed, then bisect, at most 100 steps, stop at |H - log perplexity| <= 1e-5), on the row less its
 * smallest off-diagonal entry.
 *   cond : (n, n) fp32, the normalised conditional rows at the beta returned, cond[i][i] = 0.
 *   beta : (n) fp64.             0 < perplexity < n.
 * Checks: SIMAMBA_E_SHAPE (n, perplexity), then null pointers.
 *
 * simamba_tsne_workspace_floats: host only; the floats of `ws` below for n points, SIMAMBA_E_SHAPE for an n outside the
 * limits.  ws is device memory, 16-byte aligned (else SIMAMBA_E_ALIGN; NULL: SIMAMBA_E_WORKSPACE); every word a call
 * reads from it the same call has written.
 *
 * simamba_tsne_gradient: one forces pass and the fixed-order sum; nothing moves.
 *   p         : (n, n) fp32 joint probabilities, SYMMETRIC (the kernel reads column blocks as rows), zero diagonal.
 *   y         : (n, 2) fp32.
 *   grad      : (n, 2) fp32 = 4 sum_j (exaggeration p_ij - q_ij) w_ij (y_i - y_j),  w = 1 / (1 + |y_i - y_j|^2),
 *               q = w / Z,  Z = sum_{i != j} w_ij.
 *   kl        : (1) fp64 = sum_plogp + sum_ij p_ij log(1 + |y_i - y_j|^2) + log Z  (of p itself, whatever exaggeration).
 *   sum_plogp : (1) fp64, device: the constant sum_ij p_ij log p_ij.
 * Checks: SIMAMBA_E_SHAPE (n; exaggeration not finite or <= 0), null pointers, workspace, alignment.
 *
 * simamba_tsne_run: enqueues iterations first_iter .. first_iter + n_iter - 1 of scikit-learn's _gradient_descent, two
 * launches each (forces, update) and a third on the iterations that compute the error: those with (it + 1) % 50 == 0,
 * the check iterations, and the last of the call.
 *   y, update, gains : (n, 2) fp32 state, in and out: gains += 0.2 where update * g < 0, else *= 0.8, floor 0.01;
 *                      update = momentum * update - learning_rate * gains * g;  y += update.
 *   status           : (8) fp64, in and out: [0] the last error computed (KL of exaggeration * p), [1] the gradient norm
 *                      at the last check (of gains * g, as scikit-learn takes it), [2] the best error, [3] its
 *                      iteration, [4] iterations done when [0] was written, [5] stopped, [6..7] unused.  On a check
 *                      iteration: a lower error becomes the best, otherwise it - best iteration > window stops; a
 *                      gradient norm <= min_grad_norm stops.  Every launch behind a set `stopped` returns at once.  The
 *                      caller starts a stage with [2] = DBL_MAX, [3] = first_iter, [5] = 0 (or carries them over).
 *   params           : a HOST array of four fp64 read during the call, {exaggeration > 0, 0 <= momentum < 1,
 *                      learning_rate > 0, min_grad_norm >= 0}.
 *   first_iter, n_iter, window >= 0; n_iter == 0 enqueues nothing.
 * No float atomics, every sum in a fixed order: the same bits every call.  No grid-wide barrier.
 * Checks: SIMAMBA_E_SHAPE (n, the iteration counts, then params when not NULL), null pointers, workspace, alignment;
 * all before any launch.  Still ABI version 9: symbols added, none changed.
 */
int simamba_tsne_calibrate(const float* d2, float* cond, double* beta, int n, float perplexity, void* stream);
long long simamba_tsne_workspace_floats(int n);
int simamba_tsne_gradient(const float* p, const float* y, float* grad, double* kl, float* ws, const double* sum_plogp,
                          int n, float exaggeration, void* stream);
int simamba_tsne_run(const float* p, float* y, float* update, float* gains, double* status, float* ws,
                     const double* sum_plogp, const double* params, int n, int first_iter, int n_iter, int window,
                     void* stream);

/*
 * The optimizer tail of a training step (csrc/optim.hip): gradient clipping by the global norm
 * (torch.nn.utils.clip_grad_norm_), decoupled AdamW (torch.optim.AdamW's formulation) and a per-epoch learning-rate
 * table, for any number of parameter tensors in THREE launches: the squared norm, one workgroup of scalars, the update
 * (the first is repeated once per 448 tensors beyond the first 448: a launch carries that many gradient addresses).
 * All tensors fp32.  The caller builds two tables in device memory:
 *
 *   segments : (n_segments) simamba_optim_segment, one per parameter tensor, 16-byte aligned.  p, g, exp_avg and
 *              exp_avg_sq may EACH sit at any 4-byte alignment, independently of one another (a 16-byte aligned one is
 *              accessed 16 bytes at a time).  g is WRITTEN by the call, from `grads`; the caller's value is not read.
 *              `step` is the tensor's own count of updates, fp32 as torch keeps it; the call advances it by one for
 *              every segment with a gradient.
 *   grads    : a HOST array of n_segments device addresses, read during the call: the gradient of every segment, the
 *              one column that changes from step to step.  The first kernel takes them by value and leaves them in
 *              the table, so a captured call replays with the addresses its capture saw.  NULL entry: the parameter
 *              took no gradient; all three kernels skip the segment (no decay, no step, its step count stays).
 *   first_chunk : a HOST array of n_segments + 1 ints, read during the call: segment s owns the chunk-table entries
 *              [first_chunk[s], first_chunk[s + 1]); first_chunk[0] == 0, ascending, first_chunk[n_segments] ==
 *              n_chunks (else SIMAMBA_E_SHAPE, checked when the array is not NULL).
 *   chunks   : (n_chunks, 2) int32, {segment, chunk inside the segment}: workgroup k of the first and third launch
 *              works on elements [chunk * SIMAMBA_OPTIM_CHUNK, ...) of that segment.  Every segment is covered by
 *              ceil(n / SIMAMBA_OPTIM_CHUNK) entries; 8-byte aligned.
 *   groups   : (n_groups) simamba_optim_group, 16-byte aligned.  `lr` is the address of the group's DEVICE learning
 *              rate (one fp32): read as it stands without a schedule, written with one.
 *   updates  : (1) int64, device: the count of calls so far, advanced by one.
 *   schedule : (schedule_n) fp64, device, or NULL with schedule_n == 0.  With a schedule every group runs at
 *              schedule[min(updates / steps_per_epoch, schedule_n - 1)] * lr_scale (updates as the call found it).
 *   grad_norm: (1) fp32, device, out: the norm of grad_scale * g over every segment with a gradient, before clipping.
 *   max_norm : the clip.  coef = max_norm / (grad_norm + 1e-6), clamped above at 1 with NaN propagating (a NaN norm
 *              makes every updated parameter NaN, as torch.clamp does); max_norm < 0: no clipping, coef = 1.
 *   update   : g' = grad_scale * coef * g;  p *= 1 - lr * weight_decay;  m = beta1 m + (1 - beta1) g';
 *              v = beta2 v + (1 - beta2) g'^2;  p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps).
 *              The powers, quotients and 1 - lr * weight_decay are formed in fp64, once per segment.
 *   flags    : SIMAMBA_OPTIM_ZERO_GRADS: the update also stores 0 into g in the same pass.
 *   workspace: device memory, 16-byte aligned (else SIMAMBA_E_ALIGN), at least simamba_optim_workspace_bytes() bytes
 *              (else, or NULL, SIMAMBA_E_WORKSPACE); every word a call reads from it the same call has written.
 * Limits: 1 <= n_segments <= SIMAMBA_OPTIM_MAX_SEGMENTS, 1 <= n_chunks <= SIMAMBA_OPTIM_MAX_CHUNKS (2^32 elements),
 * 1 <= n_groups <= SIMAMBA_OPTIM_MAX_GROUPS, 0 <= schedule_n <= 2^20, steps_per_epoch >= 1 with a schedule, max_norm
 * not NaN, grad_scale finite (else SIMAMBA_E_SHAPE).  The workspace query answers 0 outside [0, limit].
 * No float atomics, every sum in a fixed order: the same bits every call.
 * Checks in the order flags (SIMAMBA_E_VARIANT), shape, null pointers, workspace, alignment; all before any launch.
 * Still ABI version 9: symbols added, none changed.
 */
#define SIMAMBA_OPTIM_CHUNK 4096
#define SIMAMBA_OPTIM_MAX_SEGMENTS 65536
#define SIMAMBA_OPTIM_MAX_CHUNKS 1048576
#define SIMAMBA_OPTIM_MAX_GROUPS 256
#define SIMAMBA_OPTIM_ZERO_GRADS 1
typedef struct simamba_optim_segment {
  float* p;
  float* g;
  float* exp_avg;
  float* exp_avg_sq;
  long long n;
  int group;
  int reserved0;
  float step;
  float reserved1;
  long long reserved2;
} simamba_optim_segment;
typedef struct simamba_optim_group {
  float* lr;
  double beta1, beta2, eps, weight_decay, lr_scale;
  double reserved[2];
} simamba_optim_group;
size_t simamba_optim_workspace_bytes(int n_segments, int n_chunks);
int simamba_optim_adamw_step(void* segments, const int* chunks, const void* groups, long long* updates,
                             const double* schedule, float* grad_norm, const void* const* grads,
                             const int* first_chunk, void* workspace, size_t workspace_bytes, int n_segments,
                             int n_chunks, int n_groups, int schedule_n, int steps_per_epoch, float max_norm,
                             float grad_scale, int flags, void* stream);

/*
 * Sampling and augmentation of a batch of clouds in front of a step (csrc/augment.hip; the reference's
 * tools/runner_finetune.py:191-194 and datasets/data_transforms.py): for every cloud b and output row i < K
 *   out[b][i] = chain(points[b][ idx[b][ sel[i] ] ])
 * in one launch, one workgroup per cloud, followed by a one-lane kernel that adds 1 to the step.
 *   points   : (B, N, 3) fp32.                                        1 <= N, M, K <= 8192 ; 1 <= B < 2^31.
 *   idx      : (B, M) int32 (idx_is_64 == 0) or int64 rows into the cloud, or NULL (= the identity; then M == N).
 *   sel      : (K) int64 positions into idx's columns, shared by the batch, or NULL (= the identity; then K == M).
 *              The kernel forces every sel entry into [0, M) and every idx entry into [0, N) before it is used.
 *   lengths  : (B) int64, device, or NULL (= K everywhere): cloud b has lengths[b] output rows (clamped to [1, K] by
 *              the kernel).  Rows at and behind the length are written as 0; nothing is looked up or read for them, and
 *              flip's maximum and dropout pass them over.
 *   out      : (B, K, 3) fp32.  It may be `points` itself only when idx and sel are both NULL (in place, row for row);
 *              any other overlap of the two is refused (SIMAMBA_E_VARIANT).
 *   ops, op_params : HOST arrays of n_ops opcodes and n_ops x 4 fp32 parameters, 0 <= n_ops <= 8; read during the call:
 *     SIMAMBA_AUG_ROTATE           -                  theta = u0 * fp32(2 pi); x' = x cos - z sin, y' = y, z' = x sin + z cos
 *     SIMAMBA_AUG_SCALE            lo, hi             s_a = lo + u_a * (hi - lo);                   p'_a = p_a * s_a
 *     SIMAMBA_AUG_TRANSLATE        r                  t_a = -r + u_a * (2 r);                       p'_a = p_a + t_a
 *     SIMAMBA_AUG_SCALE_TRANSLATE  lo, hi, r          s from block 0, t from block 1;               p'_a = p_a * s_a + t_a
 *     SIMAMBA_AUG_JITTER           std, clip          p'_a = p_a + min(max(std * n_a, -clip), clip), n standard normal
 *     SIMAMBA_AUG_DROPOUT          max_ratio          ratio = u0 * max_ratio; row i becomes the cloud's current row 0
 *                                                     iff u_i <= ratio
 *     SIMAMBA_AUG_FLIP             upright axis 0|1|2 gate = u0 < 0.95; the j-th horizontal axis a (ascending) is flipped
 *                                                     iff gate and u_(1+j) < 0.5: p'_a = max_rows(p_a) - p_a (a NaN is
 *                                                     passed over by the maximum)
 *     An unknown opcode or another upright axis: SIMAMBA_E_VARIANT.
 *   state    : (2) int64, device: [seed, step].  Read by the kernel; step + 1 is written behind it in stream order.
 *              Nothing is read on the host, so the call can be captured and every replay draws anew.
 * Random numbers: Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
 *     c0 = the output row i for a per-point draw, the block number (0, 1) for a per-cloud draw
 *     c1 = the cloud b
 *     c2 = step & 0xffffffff
 *     c3 = ((step >> 32) & 0x0fffffff) | position of the op in the chain << 28 | (per-point draw ? 1 : 0) << 31
 *   so no two ops of a chain share a stream, and the result for (seed, step, b, i, chain) depends on nothing else: not
 *   on B, the launch geometry or the other clouds.  (step counts modulo 2^60.)
 *   u_k of a block = (word k >> 8) * 2^-24.  Per-cloud draws use block 0 (SCALE_TRANSLATE's t: block 1), words 0..2
 *   for the axes x, y, z.  DROPOUT's u_i is word 0 of row i's block.  JITTER's normals are Box-Muller on row i's block:
 *     n_x = R(w0) cos(2 pi u(w1)), n_y = R(w0) sin(2 pi u(w1)), n_z = R(w2) cos(2 pi u(w3)),
 *     R(w) = sqrt(-2 ln(((w >> 8) + 1) * 2^-24)).
 *   Every product and sum above is one correctly rounded fp32 operation (no contraction), so theta, s, t, ratio and the
 *   keep / flip decisions can be reproduced bit for bit; cos, sin and ln are the device library's.
 * Checks in the order shape (SIMAMBA_E_SHAPE: B, N, M, K, n_ops, M != N without idx, K != M without sel), null pointers
 * (points, out, state; ops and op_params when n_ops > 0), chain (SIMAMBA_E_VARIANT), overlap; all before any launch.
 *
 * simamba_augment_params: what the call above draws for the same chain and state, and no points; step is not advanced.
 *   cloud_params : (B, n_ops, 8) fp32; per op [theta, cos, sin] | [s_x, s_y, s_z] | [t_x, t_y, t_z] |
 *                  [s_x, s_y, s_z, t_x, t_y, t_z] | [std, clip] | [ratio] | [gate, flip_x, flip_y, flip_z] (0 / 1, the
 *                  gate already applied to the three), the rest 0.
 *   noise        : (B, K, 3) fp32 or NULL: n of the chain's FIRST jitter op (before std and the clip); 0 behind a length
 *                  or without a jitter op.
 *   keep         : (B, K) uint8 or NULL: 0 where the chain's FIRST dropout op replaces the row (u_i <= ratio) and
 *                  behind a length, else 1.
 *
 * simamba_philox4x32_10: HOST only, compiled from the header the kernels draw with: the four words of counter
 * (c0, c1, c2, c3) under the key of `seed`, into the host array out[4].
 * Still ABI version 9: symbols added, none changed.
 */
#define SIMAMBA_AUG_ROTATE          1
#define SIMAMBA_AUG_SCALE           2
#define SIMAMBA_AUG_TRANSLATE       3
#define SIMAMBA_AUG_SCALE_TRANSLATE 4
#define SIMAMBA_AUG_JITTER          5
#define SIMAMBA_AUG_DROPOUT         6
#define SIMAMBA_AUG_FLIP            7
#define SIMAMBA_AUG_MAX_OPS         8
#define SIMAMBA_AUG_CLOUD_PARAMS    8
int simamba_augment_points(const float* points, const void* idx, int idx_is_64, const long long* sel,
                           const long long* lengths, float* out, const int* ops, const float* op_params, int n_ops,
                           long long* state, long long B, int N, int M, int K, void* stream);
int simamba_augment_params(const long long* lengths, const int* ops, const float* op_params, int n_ops,
                           const long long* state, float* cloud_params, float* noise, unsigned char* keep, long long B,
                           int K, void* stream);
int simamba_philox4x32_10(long long seed, unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned* out);

/*
 * A batch out of a dataset resident on the device (csrc/dataset.hip; the reference's torch DataLoader over
 * datasets/ShapeNet55Dataset.py, ScanObjectNNDataset.py, ModelNetDataset.py and part_segmentation/dataset.py): one
 * launch, one workgroup per slot of the batch, followed by a one-lane kernel that adds 1 to the step.
 * The store:
 *   points       : (T, 3) fp32, the clouds back to back; `total` = T.
 *   offsets      : (S + 1) int64, cloud s is rows [offsets[s], offsets[s + 1]); or NULL: cloud s is rows
 *                  [s stride, (s + 1) stride), S stride <= T.  The kernel forces every range inside [0, T).
 *   labels       : (S) int64 or NULL.            point_labels : (T) int32 or NULL.
 *   state        : (2) int64 [seed, step], the layout of simamba_augment_points.  Read by the kernel; step + 1 is written
 *                  behind it in stream order.  Nothing is read on the host, so the call can be captured.
 * Which cloud goes into slot b < B:
 *   epoch = step / steps_per_epoch, pos = step % steps_per_epoch (both unsigned), p = (pos B + b) world + rank.
 *   p >= S: an empty slot (the last partial batch): index -1, label -1, length 0, rows 0; nothing is looked up.
 *   SIMAMBA_DS_SEQUENTIAL: s = p.     SIMAMBA_DS_SHUFFLE: s = perm(S, seed, stream(SHUFFLE, epoch, 0), p).
 * Which rows: the candidates are the cloud's first c = min(n_s, first) rows (first == 0: c = n_s).
 *   SIMAMBA_DS_FIRST   : row i = i, i < len = min(K, c).
 *   SIMAMBA_DS_PERMUTE : row i = perm(c, seed, stream(ROWS, epoch, p), i), i < len = min(K, c): without replacement.
 *   SIMAMBA_DS_CHOICE  : row i = (uint64(w_i) c) >> 32, i < len = K: with replacement;
 *                        w_i = word 0 of philox4x32_10(key, c0 = i, c1 = 0x80000000, c2, c3 of stream(CHOICE, epoch, p)).
 *   An empty cloud (c == 0) gives len = 0 in every mode.  Rows at and behind len are written as 0, point labels as -1.
 * Normalisation of the selected rows (datasets/ShapeNet55Dataset.py:47-53, pc_norm):
 *   SIMAMBA_DS_NONE, or SIMAMBA_DS_UNIT_SPHERE: d = row - row 0; mean_a = (sum of the len d) / len; r = d - mean;
 *   m = sqrt(max_i((r_x r_x + r_y r_y) + r_z r_z)); out = r / m.  fp32, one rounding per operation; the sum runs per lane
 *   over its rows in ascending order, over the wave by the butterfly 32 .. 1, over the waves in ascending order.  A NaN
 *   is passed over by the maximum.  Taking row 0 off first changes nothing in exact arithmetic; in fp32 it makes rows
 *   that all coincide exact zeros: then m == 0 (the reference divides by zero) and the slot is written as 0.
 * Keyed choices: perm is the bijection of csrc/keyed_perm.h (a four-round balanced Feistel network over Philox4x32-10
 * with cycle walking, stated there in full), key = (seed & 0xffffffff, seed >> 32), and
 *   stream(purpose, epoch, p) = purpose << 60 | (epoch mod 2^29) << 31 | p        (c2 = its low, c3 = its high word)
 *   purpose: SIMAMBA_DS_STREAM_SHUFFLE 1, _ROWS 2, _CHOICE 3.  Every Philox block drawn here has bit 31 of c1 set, which
 *   no block of simamba_augment_points has.
 *   So a slot's content depends only on (seed, epoch, p), the store and the modes: not on B, not on the other slots.
 * Outputs, every element written on every call:
 *   out (B, K, 3) fp32 ; index_out (B) int64 ; lengths_out (B) int32 ; label_out (B) int64 or NULL (-1 without labels) ;
 *   point_label_out (B, K) int32 or NULL (-1 without point_labels).
 * Checks in the order shape (SIMAMBA_E_SHAPE: 1 <= S < 2^31, 1 <= B < 2^31, 1 <= K <= 8192, 0 <= rank < world,
 * steps_per_epoch >= 1, first >= 0, total >= 0, without offsets 1 <= stride and S stride <= total,
 * steps_per_epoch B world <= 2^62), null pointers (points, state, out, index_out, lengths_out), modes
 * (SIMAMBA_E_VARIANT); all before any launch.
 *
 * simamba_keyed_perm: HOST only, compiled from the header the kernel uses: out[j] = perm(n, seed, stream = tweak,
 * first + j) for j < count into the host array out; 1 <= n < 2^31, first + count <= n.
 * Still ABI version 9: symbols added, none changed.
 */
#define SIMAMBA_DS_SEQUENTIAL     0
#define SIMAMBA_DS_SHUFFLE        1
#define SIMAMBA_DS_FIRST          0
#define SIMAMBA_DS_PERMUTE        1
#define SIMAMBA_DS_CHOICE         2
#define SIMAMBA_DS_NONE           0
#define SIMAMBA_DS_UNIT_SPHERE    1
#define SIMAMBA_DS_STREAM_SHUFFLE 1
#define SIMAMBA_DS_STREAM_ROWS    2
#define SIMAMBA_DS_STREAM_CHOICE  3
int simamba_dataset_fetch(const float* points, const long long* offsets, const long long* labels,
                          const int* point_labels, long long* state, float* out, long long* label_out,
                          int* point_label_out, long long* index_out, int* lengths_out, long long total, long long S,
                          long long stride, long long B, int K, int first, long long steps_per_epoch, int rank,
                          int world, int order, int rows, int norm, void* stream);
int simamba_keyed_perm(long long seed, long long tweak, long long n, long long first, long long count, long long* out);

/*
 * Damage to a batch of clouds (csrc/corrupt.hip; the families of ModelNet-C, Ren et al. 2022): one kind per call, one
 * launch, one workgroup per cloud, followed by a one-lane kernel that adds 1 to the step.
 *   points      : (B, N, 3) fp32.                                     1 <= N <= K <= 8192 ; 1 <= B < 2^31.
 *   lengths     : (B) int64, device, or NULL (= N everywhere): cloud b has n = clamp(lengths[b], 1, N) rows; the rows
 *                 behind them are never read.
 *   out         : (B, K, 3) fp32; it may not overlap points (SIMAMBA_E_VARIANT).  out_lengths : (B) int64.
 *   src         : (B, K) int32 or NULL: the input row an output row came from, or a negative code for an added row.
 *                 Rows of out at and behind out_lengths[b] are written as 0, src there as INT_MIN.
 *   state       : (2) int64 [seed, step], the layout of simamba_augment_points.  Read by the kernel; step + 1 is written
 *                 behind it in stream order.  Nothing is read on the host, so the call can be captured.
 *   kind, flags : HOST integers;  params : HOST array of 4 fp32, read during the call (unused slots are ignored).
 * Random numbers: Philox4x32-10 with the counter of simamba_augment_points at chain position 0,
 *     c0 = the block number for a per-cloud draw, the row or the added point's number for a per-point draw
 *     c1 = the cloud b ;  c2 = step & 0xffffffff ;  c3 = ((step >> 32) & 0x0fffffff) | (per-point ? 1 : 0) << 31
 *   under the key (seed & 0xffffffff, (seed >> 32) ^ SIMAMBA_CORRUPT_KEY_TWEAK): one state feeds both calls without
 *   sharing a stream.  u(w) = (w >> 8) * 2^-24; normal(block) = the three Box-Muller normals of simamba_augment_points.
 *   "cloud block k" below is per-cloud block k, "block t" per-point block t; w0..w3 are a block's words.
 * Kinds (params):
 *   DROP_GLOBAL (rho)          m = min((int)(float(n) * rho), n - 1).  Removed: the m rows with the smallest
 *                              (w0 of block i, i).  Survivors keep their order; out_len = n - m; src = the input row.
 *   DROP_LOCAL  (T, Cmax)      C = min(1 + (int)(u(cloud block 0, w0) * float(Cmax)), Cmax); T' = min(T, n - 1); cluster
 *                              j < C removes T' / C + (j < T' % C) rows, the clusters in order, each on the `a` rows
 *                              still alive: its seed is the alive row of rank min((int)(u(cloud block 1 + j, w0) *
 *                              float(a)), a - 1) in index order; removed are the alive rows with the smallest (d2, i),
 *                              d2 = (dx dx + dy dy) + dz dz in fp32 from the seed.  out_len = n - T'.
 *   ADD_GLOBAL  (A, R)         A_b = min(A, K - n) points behind the cloud's own rows, which are copied bit for bit.
 *                              Point t from block t: a = 2 u(w1), z = 1 - a, s = sqrt(a (2 - a)), phi = fp32(2 pi) u(w2),
 *                              r = R cbrt(u(w0)), p = r (s cos phi, s sin phi, z): uniform in the ball.  src = -1.
 *   ADD_LOCAL   (T, Cmax, lo, hi)  C and the cluster sizes as in DROP_LOCAL over T_b = min(T, K - n).  Cluster j: the
 *                              seed is input row min((int)(u(cloud block 1 + j, w0) * float(n)), n - 1), sigma_j = lo +
 *                              u(cloud block 1 + j, w1) * (hi - lo).  Point t belongs to the cluster whose prefix of
 *                              sizes holds t: p = seed_j + sigma_j * normal(block t).  src = -1 - j.
 *   ROTATE3     (theta)        angle_a = (2 u(cloud block 0, w_a) - 1) * theta for a = x, y, z; p' = Rz Ry Rx p.
 *   SCALE_AXES  (s >= 1)       f_a = 1 / s + u(cloud block 0, w_a) * (s - 1 / s); p'_a = p_a f_a.
 *   JITTER      (sigma)        p' = p + sigma * normal(block i); no clip.
 *   Every product, sum and quotient named above is one correctly rounded fp32 operation (no contraction) and every (int)
 *   truncates, so the counts, seeds, clusters, angles and factors can be reproduced bit for bit; cos, sin, cbrt and ln
 *   are the device library's.  Non-finite coordinates make the choice of rows unspecified and nothing else.
 * flags: SIMAMBA_CORRUPT_RENORM applies the unit-sphere normalisation of simamba_dataset_fetch to the out_len rows of
 *   the result (relative to output row 0; the sum runs per lane over its 8 consecutive rows, then as stated there).
 * The result for (seed, step, b, cloud b's rows, kind, params, N, K) depends on nothing else: not on B or the other clouds.
 * Checks in the order shape (SIMAMBA_E_SHAPE: B, N, K, K < N), null pointers (points, out, out_lengths, state, params),
 * SIMAMBA_E_VARIANT for an unknown kind or flag bit, rho outside [0, 1), a negative or NaN count, Cmax not an integer in
 * [1, 8], s < 1, then for an overlap of out and points; all before any launch.  Counts above 8192 act as 8192.
 * Still ABI version 9: symbols added, none changed.
 */
#define SIMAMBA_CORRUPT_DROP_GLOBAL  1
#define SIMAMBA_CORRUPT_DROP_LOCAL   2
#define SIMAMBA_CORRUPT_ADD_GLOBAL   3
#define SIMAMBA_CORRUPT_ADD_LOCAL    4
#define SIMAMBA_CORRUPT_ROTATE3      5
#define SIMAMBA_CORRUPT_SCALE_AXES   6
#define SIMAMBA_CORRUPT_JITTER       7
#define SIMAMBA_CORRUPT_RENORM       1
#define SIMAMBA_CORRUPT_MAX_CLUSTERS 8
#define SIMAMBA_CORRUPT_KEY_TWEAK    0x434F5252u
int simamba_corrupt_points(const float* points, const long long* lengths, float* out, long long* out_lengths, int* src,
                           long long* state, int kind, int flags, const float* params, long long B, int N, int K,
                           void* stream);

/*
 * Training-time augmentations the corruption score is lowered with (csrc/mix.hip): PointCutMix-R / -K (Zhang et al.
 * 2021) and a locally weighted deformation after PointWOLF (Kim et al. 2021).  One launch each, one workgroup per
 * output cloud, followed by a one-lane kernel that adds 1 to the step.
 *   state       : (2) int64 [seed, step], the layout of simamba_augment_points.  Read by the kernel; step + 1 is written
 *                 behind it in stream order.  Nothing is read on the host, so the calls can be captured.
 * Random numbers: the counter of simamba_corrupt_points (augment's at chain position 0; c1 = the OUTPUT cloud b) under
 *   the key (seed & 0xffffffff, (seed >> 32) ^ SIMAMBA_MIX_KEY_TWEAK), which differs from corrupt's: one state feeds
 *   augment, corrupt and mix without sharing a stream.  u(w) = (w >> 8) * 2^-24.  "cloud block k" is per-cloud block k,
 *   "block i" per-point block i; w0..w3 are a block's words.
 *   Every product, sum and quotient named below is one correctly rounded fp32 operation (no contraction) and every (int)
 *   truncates, so every discrete decision can be reproduced bit for bit; cos, sin and exp are the device library's.
 *   Non-finite coordinates make the choice of rows and anchors unspecified and nothing else.
 *
 * simamba_cutmix_points: m rows of cloud b are replaced by m rows of its partner q.
 *   points      : (B, N, 3) fp32.                                     1 <= N <= 8192 ; 1 <= B < 2^31.
 *   lengths     : (B) int64, device, or NULL (= N everywhere): cloud b has n_b = clamp(lengths[b], 1, N) rows; the rows
 *                 behind them are never read.
 *   partner     : (B) int64, device, or NULL.  Given: q = clamp(partner[b], 0, B - 1), on the device (nothing may be
 *                 read on the host).  NULL: q = perm(n = B, the key above, stream = step, b), the bijection of
 *                 csrc/keyed_perm.h: what simamba_keyed_perm(seed ^ (SIMAMBA_MIX_KEY_TWEAK << 32), step, B, b, 1, .)
 *                 answers on the host.  q == b is allowed: the result is then made of the cloud's own rows.
 *   lam         : (B) fp32, device, or NULL.  Given: lambda = lam[b] forced into [0, 1] on the device, a NaN becomes 0.
 *                 NULL: lambda = u(cloud block 0, w0).  A Beta-distributed lambda is the caller's to draw and pass in.
 *   m = min((int)(float(n_b) * lambda), n_b, n_q).      ratio : (B) fp32 out, ratio[b] = float(m) / float(n_b).
 *   out         : (B, N, 3) fp32; it may not overlap points at all (SIMAMBA_E_VARIANT): other workgroups read the
 *                 partner's rows.  Rows [0, n_b - m): the cloud's surviving rows in their input order; rows
 *                 [n_b - m, n_b): the partner's chosen rows in the partner's input order, where they are (no
 *                 translation); rows behind n_b: 0.  Copied rows are bit-for-bit copies.
 *   src         : (B, N) int32 or NULL: the own input row i (>= 0), -1 - i for partner row i, INT_MIN behind n_b.
 *   mode SIMAMBA_MIX_CUT_R: removed are the m own rows with the smallest (w0 of block i, i), taken the m partner rows
 *                 with the smallest (w1 of block i, i); both blocks under c1 = b.
 *   mode SIMAMBA_MIX_CUT_K: the own seed row is min((int)(u(cloud block 1, w0) * float(n_b)), n_b - 1), the partner's
 *                 min((int)(u(cloud block 1, w1) * float(n_q)), n_q - 1); removed are the m own rows with the smallest
 *                 (d2, i) from the own seed, taken the m partner rows with the smallest (d2, i) from the partner's seed;
 *                 d2 = (dx dx + dy dy) + dz dz in fp32 by direct differences, its bits ordered as unsigned (DROP_LOCAL).
 *   Checks in the order shape (SIMAMBA_E_SHAPE: B, N), null pointers (points, out, ratio, state), an unknown mode
 *   (SIMAMBA_E_VARIANT), an overlap of out and points (SIMAMBA_E_VARIANT); all before any launch.
 *
 * simamba_mix_draw: partner (B) int64 and / or lam (B) fp32 (either may be NULL, not both) as simamba_cutmix_points
 *   draws them from NULL at the state's present step, for the label arithmetic on top; the step is not advanced.
 *   Checks: B (SIMAMBA_E_SHAPE), state and both outputs NULL (SIMAMBA_E_NULLPTR).
 *
 * simamba_pointwolf_points: written from the paper's description, not a reproduction of its draws.
 *   points, lengths as above.  out : (B, N, 3) fp32; it may be points itself (the exact alias), any other overlap is
 *   refused (SIMAMBA_E_VARIANT).  Rows behind the length are written as 0.  1 <= M <= SIMAMBA_WOLF_MAX_ANCHORS anchors.
 *   params      : HOST array of 4 fp32 {sigma > 0, rot >= 0, scale >= 1, trans >= 0}, all finite, read during the call.
 *   anchors_out : (B, M) int32 or NULL.  Anchor 0 is row min((int)(u(cloud block 0, w0) * float(n)), n - 1); anchor k is
 *                 the row with the largest minimum d2 (as above) to anchors 0 .. k - 1, ties to the lower row.
 *   Anchor j at a_j, a = x, y, z:  angle_a = (2 u(cloud block 1 + j, w_a) - 1) * rot;
 *                 f_a = 1 + u(cloud block 9 + j, w_a) * (scale - 1), replaced by 1 / f_a when bit 31 of that block's
 *                 w3 is set (one bit for the three axes);  t_a = (2 u(cloud block 17 + j, w_a) - 1) * trans.
 *                 q_j(p) = ((Rz Ry Rx ((p - a_j) * f_j)) + a_j) + t_j, the rotation as ROTATE3 of simamba_corrupt_points.
 *   Blend:        w_j(p) = expf(-((d2(p, a_j) - min_k d2(p, a_k)) * c)), c = fp32(1 / (2 sigma^2)) formed in double on
 *                 the host and rounded once (SIMAMBA_E_VARIANT when it is not finite);
 *                 p' = (sum_j w_j q_j) / (sum_j w_j), both sums from 0 in ascending j; the nearest anchor's weight is
 *                 exp(0) = 1, so the divisor is at least 1 whatever sigma is.
 *   flags: SIMAMBA_WOLF_RENORM applies the unit-sphere normalisation of simamba_dataset_fetch to the n rows of the result
 *   (relative to row 0; the sum runs per lane over its 8 consecutive rows, then as stated there).
 *   Checks in the order shape (SIMAMBA_E_SHAPE: B, N, M), null pointers (points, out, state, params), SIMAMBA_E_VARIANT
 *   for an unknown flag bit or a parameter outside the ranges above, then for a partial overlap; all before any launch.
 * Still ABI version 9: symbols added, none changed.
 */
#define SIMAMBA_MIX_CUT_R         1
#define SIMAMBA_MIX_CUT_K         2
#define SIMAMBA_MIX_KEY_TWEAK     0x4D495847u
#define SIMAMBA_WOLF_RENORM       1
#define SIMAMBA_WOLF_MAX_ANCHORS  8
int simamba_cutmix_points(const float* points, const long long* lengths, const long long* partner, const float* lam,
                          float* out, float* ratio, int* src, long long* state, int mode, long long B, int N,
                          void* stream);
int simamba_mix_draw(long long* partner, float* lam, const long long* state, long long B, void* stream);
int simamba_pointwolf_points(const float* points, const long long* lengths, float* out, int* anchors_out,
                             long long* state, int M, const float* params, int flags, long long B, int N, void* stream);

/*
 * k-NN grouping of the tokeniser (reference models/point_mamba.py:96: pytorch3d.ops.knn_points(center, xyz,
 * K=group_size, return_sorted=False)): idx[b][g][0..K) = the K points of cloud b nearest to centre g, ascending
 * squared distance (direct differences), ties to the lower point index.
 *   points : (batch, N, 3) fp32 ; centers : (batch, G, 3) fp32 ; idx : (batch, G, K) int64.  K <= N <= 8192.
 */
int simamba_knn_group(const float* points, const float* centers, long long* idx, int batch, int N, int G, int K,
                      void* stream);
/*
 * The same for ragged batches: clouds padded to a common N, centre sets padded to a common G.
 *   len_points  : (batch) int64, device, or NULL (= N everywhere): the candidates of cloud b are its first
 *                 len_points[b] points; nothing beyond them is read.  The kernel clamps the value to [1, N]; the
 *                 library never reads it on the host.  With len_points[b] < K (K <= N still holds, else
 *                 SIMAMBA_E_SHAPE) the first len_points[b] slots of a row are its neighbours and the rest is 0.
 *   len_centers : (batch) int64, device, or NULL (= G everywhere): rows g >= len_centers[b] are not computed and are
 *                 written as 0.
 * Order within a row and the tie rule as above; every row is what simamba_knn_group returns for the cloud alone at its
 * true length.  With both pointers NULL this is simamba_knn_group (which is that call).  Still ABI version 9: symbols
 * added, none changed.
 */
int simamba_knn_group_ex(const float* points, const float* centers, const long long* len_points,
                         const long long* len_centers, long long* idx, int batch, int N, int G, int K, void* stream);

/* ---- spectral ordering ---------------------------------------------------------------- */
#define SIMAMBA_SPEC_SYMMETRIC   0x01u  /* also write A[j,i] for every kNN edge (i,j)          */
#define SIMAMBA_SPEC_SELF_LOOP   0x02u  /* keep the nearest neighbour (the point itself)        */
#define SIMAMBA_SPEC_BINARY      0x04u  /* edge weight 1 instead of exp(-alpha d^2)             */
#define SIMAMBA_SPEC_MATRIX_SYM  0x08u  /* L = I - D^-1/2 A D^-1/2, take k+1, drop the first    */
#define SIMAMBA_SPEC_SMALLEST    0x10u  /* k smallest eigenvalues (else k largest)              */
#define SIMAMBA_SPEC_SIGMA_MEAN  0x20u  /* weight exp(-d^2 / 2 sigma^2), sigma = mean distance
                                           over the whole batch (reference alpha == 0 branch)  */
#define SIMAMBA_SPEC_LARGE_G     0x40u  /* simamba_laplacian_topk_ex only: run the large-G kernel at
                                           G <= 128 too (parity tests; production leaves it 0) */

/*
 * k-NN graph adjacency.  points (B,G,F) fp32 -> adj (B,G,G) fp32, 2 <= G <= 512 (above 128: two launches over
 * row blocks, the adjacency zero-filled in place; the same edges and weights as the G <= 128 kernel).
 * workspace: >= 256 bytes (used by SIGMA_MEAN only).
 */
int simamba_knn_graph(const float* points, float* adj, void* workspace, size_t ws_bytes,
                      int B, int G, int F, int knn, float alpha, unsigned flags, void* stream);

/*
 * Laplacian eigen-decomposition, one workgroup per sample (cyclic Jacobi, LDS-resident), 2 <= G <= 128.
 *   adj        : (B,G,G) fp32
 *   evals      : (B,k)      evecs : (B,G,k)      order : (B,k,G) int64 (ascending argsort of
 *                each selected eigenvector, ties by index); any of the three may be NULL.
 *   all_evals  : (B,G) ascending, all_evecs : (B,G,G) columns = eigenvectors; may be NULL.
 * Reproduces the reference's quirk of decomposing the LOWER TRIANGLE of I - D^-1 A.
 * Eigenvector sign: the component of largest magnitude is made positive (LAPACK/cuSOLVER
 * leave the sign unspecified).
 */
int simamba_laplacian_topk(const float* adj, float* evals, float* evecs, long long* order,
                           float* all_evals, float* all_evecs, int B, int G, int k,
                           unsigned flags, void* stream);

/*
 * Top-k eigenpairs for 2 <= G <= 512: the contract of simamba_laplacian_topk without the full-spectrum outputs.
 * G <= 128 (and SIMAMBA_SPEC_LARGE_G clear): exactly simamba_laplacian_topk(..., NULL, NULL, ...); the workspace
 * is not used and may be NULL.  Above 128 (or with SIMAMBA_SPEC_LARGE_G): Householder tridiagonalisation with the
 * matrix in `workspace` (>= simamba_laplacian_topk_workspace_bytes(B,G) bytes, one G x G fp32 matrix per sample),
 * fp64 bisection and inverse iteration; k (+1 for MATRIX_SYM) <= 8.  Unknown flag bits: SIMAMBA_E_VARIANT.
 */
size_t simamba_laplacian_topk_workspace_bytes(int B, int G);
int simamba_laplacian_topk_ex(const float* adj, float* evals, float* evecs, long long* order,
                              void* workspace, size_t ws_bytes, int B, int G, int k, unsigned flags,
                              void* stream);

/* 256 + 4*B*G*G for G <= 128; above, the large-G eigensolver's workspace is appended (256-byte aligned). */
size_t simamba_spectral_workspace_bytes(int B, int G);

/* centres (B,G,3) -> top-k eigenpairs + orders, 2 <= G <= 512; workspace holds the (B,G,G) adjacency (and above
 * 128 the eigensolver's matrix). */
int simamba_spectral_topk(const float* centers, float* evals, float* evecs, long long* order,
                          void* workspace, size_t ws_bytes, int B, int G, int knn, float alpha,
                          int k, unsigned flags, void* stream);

/*
 * Space-filling-curve orders of the centres (an extension: the reference has none; the Hilbert / trans-Hilbert and
 * Z-order serialisations its method is measured against, in the (B,k,G) form of the spectral orders).  One launch,
 * one workgroup per cloud and curve, 2 <= G <= 8192, 1 <= k <= 8 curves, 1 <= bits <= 16 per axis.
 *   centers : (B,G,3) fp32
 *   curves  : k curve ids, on the HOST (read before the launch, never after the call returns)
 *   order   : (B,k,G) int64: the patches of cloud b along curve c, ascending by (code, patch index)
 *   codes   : (B,k,G) int64 or NULL: codes[b,c,g] = the code of patch g on curve c (by patch, not in sorted order)
 *   box     : SIMAMBA_CURVE_BOX_CLOUD: lo_a = the minimum of axis a, ext = the largest of the three extents max_a -
 *             min_a (fp32), both over the finite coordinates of the cloud (an axis without one: lo_a = 0, extent 0);
 *             box_lo / box_hi are ignored.  SIMAMBA_CURVE_BOX_FIXED: lo_a = box_lo, ext = box_hi - box_lo (fp32) for
 *             every cloud and axis.
 * Cell of a coordinate x on axis a, in float64: q = floor(((double)x - (double)lo_a) / (double)ext * 2^bits), clamped
 * to [0, 2^bits - 1]; a non-finite x: 2^bits - 1; else ext == 0: 0.  Code of a cell (q_x, q_y, q_z): _Z the bit
 * interleave (bit i of x, y, z at bits 3i+2, 3i+1, 3i), _HILBERT Skilling's transpose algorithm on (x, y, z) read out
 * with the same interleave; with _TRANS both run on (y, x, z).
 * Checks in the order shape (SIMAMBA_E_SHAPE: B < 0, G, k, bits), null pointers (centers, curves, order), box mode and
 * curve ids (SIMAMBA_E_VARIANT), fixed box (SIMAMBA_E_SHAPE: box_lo or box_hi not finite, box_lo >= box_hi); all
 * before any launch.  B == 0: SIMAMBA_OK, nothing read.  Still ABI version 9: symbols added, none changed.
 */
#define SIMAMBA_CURVE_Z             0
#define SIMAMBA_CURVE_HILBERT       1
#define SIMAMBA_CURVE_TRANS         2   /* or-ed into _Z / _HILBERT: the curve on (y, x, z) */
#define SIMAMBA_CURVE_Z_TRANS       2
#define SIMAMBA_CURVE_HILBERT_TRANS 3
#define SIMAMBA_CURVE_BOX_CLOUD     0
#define SIMAMBA_CURVE_BOX_FIXED     1
int simamba_curve_order(const float* centers, const int* curves, long long* order, long long* codes,
                        int B, int G, int k, int bits, int box, float box_lo, float box_hi, void* stream);

/*
 * Farthest-point sampling (tokeniser step ahead of the hot path; replaces
 * pytorch3d.ops.sample_farthest_points at reference models/point_mamba.py:93).
 *   points (B, N, 3) fp32 -> idx (B, K) int64 (first pick = point 0, ties to the lower index),
 *   centers (B, K, 3) fp32 or NULL.  N <= 8192 (a 1024-lane kernel above 4096), K <= N.
 */
int simamba_farthest_point_sample(const float* points, long long* idx, float* centers, int B, int N,
                                  int K, void* stream);
/*
 * The same for ragged batches: clouds padded to a common N.
 *   lengths : (B) int64, device, or NULL (= N everywhere): cloud b consists of its first lengths[b] points; nothing
 *             beyond them is read, so the padding may hold anything (NaN, Inf).  The kernel clamps the value to
 *             [1, N]; the library never reads it on the host.
 *   start   : (B) int64, device, or NULL (= point 0): the first pick of cloud b, 0 <= start[b] < lengths[b] (clamped
 *             into that range by the kernel).
 * K <= N as above (else SIMAMBA_E_SHAPE); K > lengths[b] is legal: min(K, lengths[b]) picks are made, the remaining idx
 * slots are written as -1 and the remaining centers rows as 0.  The picks are those of simamba_farthest_point_sample
 * on the cloud alone at its true length.  With both pointers NULL this is simamba_farthest_point_sample (which is that
 * call).  Still ABI version 9.
 */
int simamba_farthest_point_sample_ex(const float* points, const long long* lengths, const long long* start,
                                     long long* idx, float* centers, int B, int N, int K, void* stream);

/* vals (rows, n) fp32 -> idx (rows, n) int64, ascending, ties by index.  n <= 1024. */
int simamba_argsort_rows(const float* vals, long long* idx, int rows, int n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SIMAMBA_H_ */
