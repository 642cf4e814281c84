/* libdlwpmi — MI355X (gfx950) native kernels for the dlwp-benchmark autoregressive rollout
 * training path.  C ABI: plain pointers and sizes, no torch types.
 *
 * The reference (amazon-science/dlwp-benchmark) has no FFI of its own: its boundary is the
 * Python nn.Module surface.  Each entry point below therefore names the
 * reference call it replaces (file:line under /root/reference/src); the Python host side
 * in dlwp_benchmark_amd/ binds them with ctypes and re-exposes the reference's module
 * constructors / forward signatures.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer borrowed from the caller (never freed or retained
 *     beyond the call, except buffers explicitly bound to a trainer);
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued there, no hidden
 *     synchronisation (graph-capture safe) unless a function says otherwise;
 *   - return 0 on success, negative DLWP_E_* on failure; dlwp_last_error() gives the
 *     thread-local message;
 *   - arithmetic: IEEE fp32 on the exact-f32 MFMA by default (the reference's fp32 path: the FNO rollout kernels, the GEMMs
 *     under dlwp_set_gemm_precision(0), the FFT and SHT kernels without a _bf16 suffix); bf16 OPERANDS with fp32 accumulation,
 *     epilogues and statistics where the reference trains under bf16 autocast (BASELINE configs C3-C5): dlwp_set_gemm_precision(1),
 *     the *_mixed GEMM entries (bf16 arrays in HBM), and the entry points that say so (dlwp_sfno_tail_*, dlwp_sfno_encode_* /
 *     _decode_*, dlwp_sht_*_bf16, dlwp_wgrad_segments);
 *   - scratch: entry points that need a workspace take it from the caller (dlwp_*_workspace_bytes + a pointer).  Two older ones
 *     keep a library-owned slab per device instead (the sliced weight-gradient GEMM, dlwp_sumsq's partials): grow-only,
 *     allocated outside stream captures only, never freed or re-used for anything else while the process lives.
 */
#ifndef DLWPMI_H
#define DLWPMI_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DLWPMI_VERSION 100

#define DLWP_OK 0
#define DLWP_E_INVALID (-1)
#define DLWP_E_HIP (-2)
#define DLWP_E_UNSUPPORTED (-3)
#define DLWP_E_NOMEM (-4)

int dlwp_version(void);
const char* dlwp_last_error(void);

/* Measurement knobs (csrc/tuning.hip): every override of a dispatch heuristic -- kernel family, tile size, workgroup count -- is a   */
/* named entry of ONE registry.  dlwp_set_tuning(name, value) sets an override (name with or without the "DLWP_" prefix of the     */
/* environment variable of the same meaning), dlwp_clear_tuning(name) removes it (NULL: all); while no override is set the            */
/* environment variable DLWP_<NAME> is consulted at the time of use.  Unset = the library's own choice.  No knob changes results     */
/* beyond summation order.  dlwp_get_tuning returns 1 and the value when an override (either kind) is in force, else 0;             */
/* dlwp_tuning_list(i, &name, &doc) enumerates the registry (returns 0 past the end).                                               */
int dlwp_set_tuning(const char* name, int value);
int dlwp_clear_tuning(const char* name);
int dlwp_get_tuning(const char* name, int* value);
int dlwp_tuning_list(int index, const char** name, const char** doc);

/* Live per-kernel accounting (csrc/prof.hip; measurement only, no reference counterpart: the reference times whole epochs with    */
/* time.time(), src/nsbench/scripts/train.py:108,164).  Between dlwp_prof_enable(1) and dlwp_prof_collect() every instrumented      */
/* launch (the GEMM families, window attention, LayerNorm, segmented weight gradients, FFT passes) is bracketed by two HIP events    */
/* on its own stream and recorded with its kernel name, algorithmic flops and algorithmic HBM bytes (from the launch arguments).    */
/* Not recorded under stream capture.  dlwp_prof_collect() blocks until the recorded events have completed, folds the records by    */
/* kernel name, sorts by total time and returns the number of rows; dlwp_prof_get(i, ...) reads row i (name truncated to name_len). */
/* dlwp_prof_enable(2): the GEMM rows also carry the product's shape and epilogue in their name (one row per distinct product).    */
int dlwp_prof_enable(int on);
int dlwp_prof_collect(void);
int dlwp_prof_get(int index, char* name, int name_len, long long* calls, double* ms, double* flops, double* bytes);

/* ------------------------------------------------------------------------------------ */
/* Strided / gathered channel views.  A rollout step reads its input channels straight   */
/* out of the trajectory buffers (observations or earlier predictions) instead of        */
/* re-stacking them (reference: th.stack/th.cat per step, nsbench/models/fno/fno.py:     */
/* 228-237).  Either (base,bstride,cstride) or a per-channel pointer table is used.      */
typedef struct dlwp_chan_src {
    const float* base;
    long long bstride, cstride;        /* elements */
    const float* const* tab;           /* device array [C] of sample-0 plane pointers    */
    const long long* tab_bstride;      /* device array [C] of batch strides (elements)   */
} dlwp_chan_src;
typedef struct dlwp_chan_dst {
    float* base;
    long long bstride, cstride;
    float* const* tab;                 /* entries may be NULL: channel skipped           */
    const long long* tab_bstride;
} dlwp_chan_dst;

/* ------------------------------------------------------------------------------------ */
/* Pointwise 2-layer channel MLP: y = W2 gelu(W1 x + b1) + b2 on [B,C,P] fields.         */
/* Replaces neuralop FNO.lifting / FNO.projection (constructed at nsbench/models/fno/    */
/* fno.py:19-27,205-215; dlwpbench/models/fno/fno.py:38-47).  w1:[Ch,Cin] b1:[Ch]        */
/* w2:[Cout,Ch] b2:[Cout] (Conv2d 1x1 weight layout).                                    */
int dlwp_pwmlp_fwd(const float* x, const float* w1, const float* b1, const float* w2,
                   const float* b2, float* y, int B, int Cin, int Ch, int Cout, int P,
                   void* stream);
/* gx may be NULL. gw1,gb1,gw2,gb2 are ACCUMULATED into (caller zeroes them).            */
int dlwp_pwmlp_bwd(const float* x, const float* w1, const float* b1, const float* w2,
                   const float* gy, float* gx, float* gw1, float* gb1, float* gw2, float* gb2,
                   int B, int Cin, int Ch, int Cout, int P, void* stream);

/* Variant used inside the rollout: parameter gradients are written to a per-workgroup     */
/* partial slab of dlwp_pwmlp_slab_floats() floats (plain stores when slab_accumulate == 0, */
/* read-modify-write by the owning workgroup otherwise: deterministic, not bound by the     */
/* chip-wide float-atomic rate) and folded into the gradients by dlwp_pwmlp_slab_fold.      */
long long dlwp_pwmlp_slab_floats(int B, int Cin, int Ch, int Cout, int P);
int dlwp_pwmlp_bwd_slab(const float* x, const float* w1, const float* b1, const float* w2,
                        const float* gy, float* gx, float* slab, int slab_accumulate, int B,
                        int Cin, int Ch, int Cout, int P, void* stream);
int dlwp_pwmlp_slab_fold(const float* slab, float* gw1, float* gb1, float* gw2, float* gb2, int B,
                         int Cin, int Ch, int Cout, int P, void* stream);

/* ------------------------------------------------------------------------------------ */
/* FNO block: pre = irfft2(W . trunc(rfft2(act(x)))) + Wskip act(x) + bias               */
/* (neuralop FNOBlocks: SpectralConv + linear skip; call sites        */
/* `self.fno(x_t)` nsbench/models/fno/fno.py:38,96,246, dlwpbench/models/fno/fno.py:103). */
/* The mode-truncated transform is a pruned DFT (two small GEMMs per axis) fused with     */
/* the skip GEMM; no full spectrum is ever formed.                                        */
/*   x, pre : [B,C,H,W];  act_in!=0 applies GELU to x on load (x is then the previous     */
/*            block's pre-activation);                                                    */
/*   wspec  : [m1][m2c][Cin][Cout][2] (mode-major complex; m2c = n_modes[1]/2+1);         */
/*   wskip  : [Cout][Cin]; bias : [C];                                                    */
/*   xhat   : [B][m1][m2c][C][2] truncated spectrum of act(x), saved for backward.        */
typedef struct dlwp_fno_plan dlwp_fno_plan;
int dlwp_fno_plan_create(int C, int H, int W, int m1, int m2c, dlwp_fno_plan** out);
/* 3-D (time, y, x) blocks on [B,C,T,H,W] volumes (nsbench FNOContextModule / neuralop FNO with three n_modes): the plan  */
/* treats the volume as a (T*H) x W image with m0*m1 kept row frequencies (separable product twiddles); x, pre:            */
/* [B,C,T*H,W]; wspec [m0*m1][m2c][Cin][Cout][2]; xhat [B][m0*m1][m2c][C][2].                                             */
int dlwp_fno_plan_create3d(int C, int T, int H, int W, int m0, int m1, int m2c, dlwp_fno_plan** out);
void dlwp_fno_plan_destroy(dlwp_fno_plan* plan);
/* bytes of scratch the block calls need for batch B (caller allocates, 256-B aligned)   */
size_t dlwp_fno_block_workspace_bytes(const dlwp_fno_plan* plan, int B);
int dlwp_fno_block_fwd(const dlwp_fno_plan* plan, const float* x, int act_in, const float* wspec,
                       const float* wskip, const float* bias, float* pre, float* xhat, int B,
                       void* workspace, void* stream);
/* g_x = d loss / d x (includes the GELU derivative when act_in). g_wspec/g_wskip/g_bias */
/* are ACCUMULATED into.                                                                  */
int dlwp_fno_block_bwd(const dlwp_fno_plan* plan, const float* x, int act_in, const float* wspec,
                       const float* wskip, const float* g_pre, const float* xhat, float* g_x,
                       float* g_wspec, float* g_wskip, float* g_bias, int B, void* workspace,
                       void* stream);
/* The same backward as the rollout trainer runs it (narrow layers, hidden_channels <= 64): the skip-weight and bias    */
/* gradients go into a per-workgroup partial slab of dlwp_fno_block_slab_floats() floats (plain stores when           */
/* slab_accumulate == 0, read-modify-write by the owning workgroup otherwise: deterministic, no same-address float     */
/* atomics) and dlwp_fno_block_slab_fold ACCUMULATES the folded slab into g_wskip / g_bias.                            */
long long dlwp_fno_block_slab_floats(const dlwp_fno_plan* plan, int B);
int dlwp_fno_block_bwd_slab(const dlwp_fno_plan* plan, const float* x, int act_in, const float* wspec,
                            const float* wskip, const float* g_pre, const float* xhat, float* g_x,
                            float* g_wspec, float* slab, int slab_accumulate, int B, void* workspace,
                            void* stream);
int dlwp_fno_block_slab_fold(const dlwp_fno_plan* plan, const float* slab, float* g_wskip, float* g_bias,
                             int B, void* stream);
/* dlwp_fno_block_bwd_slab as the rollout trainer runs a block by default: the slab is formed by extra workgroups of the     */
/* per-mode launch (fno_mix_bwd_skipgrad_kernel) and the `spatial` launch behind it runs without by-products.  Every output   */
/* bit for bit dlwp_fno_block_bwd_slab's.  DLWP_E_UNSUPPORTED, nothing launched, for wide / 3-D plans, for shapes whose        */
/* backward `spatial` keeps its four-wave kernel (C_pad 64 on 64-wide rows), or with the knob FNO_SKIP_WGRAD_IN_MIX = 0.      */
int dlwp_fno_block_bwd_slab_split(const dlwp_fno_plan* plan, const float* x, int act_in, const float* wspec,
                                  const float* wskip, const float* g_pre, const float* xhat, float* g_x,
                                  float* g_wspec, float* slab, int slab_accumulate, int B, void* workspace,
                                  void* stream);
/* The backward of the FIRST block (its input h0 = the lifting MLP's output, not activated) fused with the lifting MLP's      */
/* backward: rows DFT, per-mode stage, then ONE launch for `spatial` + the MLP backward -- the gradient of h0 stays in LDS and  */
/* is never written.  Outputs bit for bit those of dlwp_fno_block_bwd_slab(act_in = 0) followed by dlwp_pwmlp_bwd_slab on its   */
/* g_x: g_wspec, the skip slab (dlwp_fno_block_slab_fold), the lifting slab (dlwp_pwmlp_slab_fold; Cout = the plan's C,         */
/* P = H * W) and gx.  x, gx: dense [B][Cin][H W]; gx nullable, gx_accumulate != 0 adds to it; each slab has its own            */
/* accumulate flag.  DLWP_E_UNSUPPORTED, nothing launched, where the library itself takes the two launches: rows that are not  */
/* 64 wide, more than 48 channels, wide / 3-D plans, Cin > 32 (Cin > 16 for at most 16 channels), or the knob                  */
/* FNO_FUSE_LIFT_BWD = 0.                                                                                                      */
int dlwp_fno_block_lift_bwd_slab(const dlwp_fno_plan* plan, const float* h0, const float* wspec, const float* wskip,
                                 const float* g_pre, const float* xhat, float* g_wspec, float* slab_skip,
                                 int slab_skip_accumulate, const float* x, const float* w1, const float* b1,
                                 const float* w2, float* gx, int gx_accumulate, float* slab_lift,
                                 int slab_lift_accumulate, int B, int Cin, int Ch, void* workspace, void* stream);

/* dlwp_fno_block_lift_bwd_slab with a third phase in the same launch: the scalar-output projection backward of the PREVIOUS net  */
/* call of a rollout, which works on the same 64-pixel rows and needs from this launch only its own rows of the closed-loop       */
/* gradient.  px [B][C][H W]: that call's last `pre`; pw1 [PCh][C], pb1 [PCh], pw2 [PCout][PCh]; gy: one [H W] plane per sample,  */
/* gy_bstride floats apart -- in the rollout a plane of the tensor gx accumulates into (gx_accumulate != 0), read after this      */
/* launch's own additions; pred, target [B][PCout][H W]: upstream = gy + mse_scale * (pred - target); gcur [B][C][H W] and        */
/* x1_out [B][H][m2c][C] complex (its adjoint rows DFT) are overwritten; slab_proj: dlwp_pwmlp_slab_floats(B, C, PCh, PCout, H W). */
/* Outputs bit for bit those of dlwp_fno_block_lift_bwd_slab followed by dlwp_pwmlp_proj_bwd_rows_slab.  DLWP_E_UNSUPPORTED,       */
/* nothing launched, where the library keeps that launch: whatever dlwp_fno_block_lift_bwd_slab refuses, PCout != 1, gres != NULL */
/* (a residual path), more than 32 channels, more than 8 kept column frequencies, or the knob FNO_FUSE_PROJ_BWD = 0.              */
int dlwp_fno_block_lift_proj_bwd_slab(const dlwp_fno_plan* plan, const float* h0, const float* wspec, const float* wskip,
                                      const float* g_pre, const float* xhat, float* g_wspec, float* slab_skip,
                                      int slab_skip_accumulate, const float* x, const float* w1, const float* b1,
                                      const float* w2, float* gx, int gx_accumulate, float* slab_lift,
                                      int slab_lift_accumulate, int B, int Cin, int Ch, const float* px, const float* pw1,
                                      const float* pb1, const float* pw2, const float* gy, long long gy_bstride,
                                      const float* pred, const float* target, float mse_scale, const float* gres, float* gcur,
                                      float* x1_out, float* slab_proj, int slab_proj_accumulate, int PCh, int PCout,
                                      void* workspace, void* stream);
/* The projection backward as the rollout trainer issues it on its own launch (slab mode, MSE term, adjoint rows DFT of the       */
/* finished gradient rows where the shapes allow, else a separate rows launch): the reference of the entry point above.           */
int dlwp_pwmlp_proj_bwd_rows_slab(const dlwp_fno_plan* plan, const float* px, const float* pw1, const float* pb1,
                                  const float* pw2, const float* gy, long long gy_bstride, const float* pred,
                                  const float* target, float mse_scale, float* gcur, float* x1_out, float* slab_proj,
                                  int slab_proj_accumulate, int B, int PCh, int PCout, void* stream);

/* The forward of the LAST block fused with the projection MLP on its result, as the training rollout runs it: rows DFT,         */
/* per-mode stage, then ONE launch for `spatial` + projection (+ the next net call's lifting MLP with its rows DFT) -- the row  */
/* `spatial` finishes in LDS is the projection's input tile; pre is written, not read back.  pre, xhat as dlwp_fno_block_fwd;   */
/* frame [B][Cout1][H W] = projection(pre) (+ res, nullable, frame's layout).  window != NULL adds the second MLP:              */
/* h0_next [B][C][H W] = lifting(window [B][Cin2][H W], whose channel next_ch[o] >= 0 (host array of 8) is taken from frame      */
/* channel o in LDS and not read) and x1_next [B][H][m2c][C][2] its W-axis DFT.  Outputs bit for bit those of                   */
/* dlwp_fno_block_fwd followed by dlwp_pwmlp_proj_lift_fwd (the two-launch form on the same tensors: pwmlp_fwd_chain_kernel, or */
/* pwmlp_fwd_kernel without a window).  DLWP_E_UNSUPPORTED, nothing launched, where the library keeps the two launches: rows    */
/* that are not 64 wide, more than 48 channels (32 with a window, which also needs m2c <= 8), wide / 3-D plans, Cout1 > 8,       */
/* shapes the chained launch refuses, more than 160 KiB of LDS, or the knob FNO_FUSE_PROJ_FWD = 0.                              */
int dlwp_fno_block_proj_fwd(const dlwp_fno_plan* plan, const float* x, int act_in, const float* wspec, const float* wskip,
                            const float* bias, float* pre, float* xhat, const float* pw1, const float* pb1, const float* pw2,
                            const float* pb2, const float* res, float* frame, int Ch1, int Cout1, const float* window,
                            const float* lw1, const float* lb1, const float* lw2, const float* lb2, float* h0_next,
                            float* x1_next, int Cin2, int Ch2, const signed char* next_ch, int B, void* workspace, void* stream);
int dlwp_pwmlp_proj_lift_fwd(const dlwp_fno_plan* plan, const float* pre, const float* pw1, const float* pb1, const float* pw2,
                             const float* pb2, const float* res, float* frame, int Ch1, int Cout1, const float* window,
                             const float* lw1, const float* lb1, const float* lw2, const float* lb2, float* h0_next,
                             float* x1_next, int Cin2, int Ch2, const signed char* next_ch, int B, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Training-step pieces (nsbench/scripts/train.py:113-131: MSELoss, Adam).               */
/* loss_out (device, 1 float) += sum((a-b)^2) * scale                                    */
int dlwp_sqerr_sum(const float* a, const float* b, long long n, float scale, float* loss_out,
                   void* stream);
/* nn.MSELoss forward + backward in one pass (train.py:113,119-122):                      */
/* loss_out (device, 1 float) += mean((pred-target)^2); grad = 2 (pred-target) / n        */
int dlwp_mse_fwd_bwd(const float* pred, const float* target, long long n, float* loss_out,
                     float* grad, void* stream);
/* Evaluation metrics (nsbench/scripts/evaluate.py:232-257: RMSE / accumulated error per time */
/* step; dlwpbench/scripts/evaluate.py:494-546: latitude-weighted RMSE and ACC per (time,      */
/* variable)).  out/target/climatology are [B][G][H][W]; row_weights [H] or NULL (= 1);         */
/* climatology may be NULL.  moments [5][G] (device) is ACCUMULATED into:                       */
/*   sum w (o-t)^2 | sum w |o-t| | sum w (o-c)(t-c) | sum w (o-c)^2 | sum w (t-c)^2             */
int dlwp_error_moments(const float* out, const float* target, const float* climatology,
                       const float* row_weights, int B, int G, int H, int W, float* moments,
                       void* stream);
/* torch.optim.Adam (no weight decay / amsgrad) on a flat buffer; `step` is a device      */
/* int32 counter incremented by the kernel; grads are multiplied by grad_scale first      */
/* (1/world_size after a sum all-reduce) and zeroed afterwards when zero_grad != 0.       */
int dlwp_adam_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int* step,
                   long long n, float lr, float beta1, float beta2, float eps, float grad_scale,
                   int zero_grad, void* stream);
/* The same step with torch.nn.utils.clip_grad_norm_ folded in (dlwpbench scripts/train.py:133-135 clips at  */
/* max_norm = learning rate before optimizer.step()): sumsq (device float, sum(g^2) of the UNSCALED gradient */
/* as dlwp_sumsq leaves it; NULL = no clipping) gives the coefficient min(1, max_norm / (sqrt(*sumsq) *       */
/* |grad_scale| + 1e-6)) that multiplies the gradient as Adam reads it -- the gradient buffer is not         */
/* rewritten (no dlwp_clip_scale pass): use it when the clipped gradient itself is not needed afterwards.    */
int dlwp_adam_step_clipped(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int* step,
                           long long n, float lr, float beta1, float beta2, float eps, float grad_scale,
                           int zero_grad, const float* sumsq, float max_norm, void* stream);
/* out (device float) = sum(g^2)   (for clip_grad_norm_, train.py:123-125)                */
int dlwp_sumsq(const float* g, long long n, float* out, void* stream);
/* g *= min(1, max_norm / (sqrt(*sumsq * grad_scale^2) + 1e-6))  (torch clip_grad_norm_)  */
int dlwp_clip_scale(float* g, long long n, const float* sumsq, float grad_scale, float max_norm,
                    void* stream);

/* ------------------------------------------------------------------------------------ */
/* Fused FNO rollout trainer: the whole autoregressive rollout forward, MSE, and BPTT     */
/* backward of nsbench TFNO2DModule / FNOModule (fno.py:29-41,217-250) and of the         */
/* residual dlwpbench form (dlwpbench/models/fno/fno.py:64-106), captured into one        */
/* hipGraph.  Parameters/gradients live in ONE flat fp32 buffer owned by the caller       */
/* (layout: dlwp_fno_param_offset); the gradient buffer is what data-parallel ranks        */
/* all-reduce (one flat RCCL bucket).                                                     */
typedef struct dlwp_fno_cfg {
    int B, T, D;            /* batch, sequence length, channels per frame (ns: D=1)       */
    int H, W;
    int context_size;       /* ctx frames flattened into channels (TFNO2DModule); 0/1:    */
                            /* FNOModule single-frame form                                 */
    int teacher_forcing_steps;
    int hidden, lifting, projection, n_layers;
    int m1, m2c;            /* kept modes: n_modes[0] rows, n_modes[1]/2+1 columns        */
    int out_channels;       /* = D                                                         */
    int form;               /* DLWP_FNO_FORM_NS: nsbench fno.py:217-250 (x[B,T,D,H,W] -> [B,T,D,H,W]);    */
                            /* DLWP_FNO_FORM_DLWP: dlwpbench fno.py:64-106 (D = prognostic channels,      */
                            /* out[k] = last frame + net([constants|prescribed|prognostic window]),       */
                            /* k = 0..T-ctx-1, teacher_forcing_steps unused)                              */
    int constant_channels;  /* dlwp form: channels of constants [B,1,Cc,H,W]                              */
    int prescribed_channels;/* dlwp form: channels of prescribed [B,T,Cp,H,W]                             */
    int m0;                 /* DLWP_FNO_FORM_NS_CONTEXT3D: kept TEMPORAL modes n_modes[0] (m1 = n_modes[1] rows,  */
                            /* m2c = n_modes[2]/2+1 columns); 0 for the 2-D forms                                 */
} dlwp_fno_cfg;
#define DLWP_FNO_FORM_NS 0
#define DLWP_FNO_FORM_DLWP 1
/* nsbench FNOContextModule (fno.py:44-100): the context window [B, ctx, D, H, W] is a [B, D, ctx, H, W] VOLUME for a     */
/* 3-D (time, y, x) FNO and the last time slice of the result is the prediction; context_size = n_modes[0] (:54).         */
/* The (time, y) transform pair is one dense separable DFT: the block kernels see a (ctx*H) x W image with m0*m1 kept     */
/* "row" frequencies whose twiddles are products e^{-2 pi i (kt t/ctx + ky h/H)}; spectral weights [m0*m1][m2c][C][C][2].  */
#define DLWP_FNO_FORM_NS_CONTEXT3D 2

enum {
    DLWP_FNO_P_LIFT_W1 = 0, DLWP_FNO_P_LIFT_B1, DLWP_FNO_P_LIFT_W2, DLWP_FNO_P_LIFT_B2,
    DLWP_FNO_P_PROJ_W1, DLWP_FNO_P_PROJ_B1, DLWP_FNO_P_PROJ_W2, DLWP_FNO_P_PROJ_B2,
    DLWP_FNO_P_SPEC_W,   /* + layer: [m1][m2c][C][C][2]  */
    DLWP_FNO_P_SKIP_W,   /* + layer: [C][C]              */
    DLWP_FNO_P_SPEC_B    /* + layer: [C]                 */
};
/* element offset and size of a parameter tensor inside the flat buffer; total = offset   */
/* returned for kind = -1.                                                                */
long long dlwp_fno_param_offset(const dlwp_fno_cfg* cfg, int kind, int layer, long long* size);

typedef struct dlwp_fno_trainer dlwp_fno_trainer;
int dlwp_fno_trainer_create(const dlwp_fno_cfg* cfg, dlwp_fno_trainer** out);
void dlwp_fno_trainer_destroy(dlwp_fno_trainer* tr);
/* bind the caller's trajectory buffers (borrowed): x [B,T,D,H,W] observations, y targets  */
/* (may be NULL when only forward / backward(grad_out) are used), out predictions, loss     */
/* (1 device float: mean squared error, may be NULL likewise).  Synchronous (uploads the    */
/* channel gather tables); invalidates a captured graph.                                    */
int dlwp_fno_trainer_bind_io(dlwp_fno_trainer* tr, const float* x, const float* y, float* out,
                             float* loss);
/* dlwp form only, BEFORE bind_io: constants [B,1,Cc,H,W] and prescribed [B,T,Cp,H,W]     */
/* (NULL when the corresponding channel count is 0).  In the dlwp form x is the prognostic */
/* trajectory [B,T,Cg,H,W] and y/out are [B,T-ctx,Cg,H,W].                                 */
int dlwp_fno_trainer_bind_aux(dlwp_fno_trainer* tr, const float* constants, const float* prescribed);
/* bind the caller's flat parameter / gradient buffers (borrowed until destroy/rebind)    */
int dlwp_fno_trainer_bind(dlwp_fno_trainer* tr, float* params, float* grads);
/* rollout forward into the `out` buffer; keep_activations!=0 stores every net call's      */
/* activations for a following dlwp_fno_trainer_backward (0: evaluation)                   */
int dlwp_fno_trainer_forward(dlwp_fno_trainer* tr, int keep_activations, void* stream);
/* BPTT backward of the last kept forward.  grad_out = d loss / d out [B,T,D,H,W], or NULL */
/* for the fused nn.MSELoss(mean) against the `y` buffer (loss value -> `loss` buffer).    */
/* Parameter gradients are ACCUMULATED into the bound gradient buffer.                     */
int dlwp_fno_trainer_backward(dlwp_fno_trainer* tr, const float* grad_out, void* stream);
/* forward(keep) + backward(NULL) in one call.                                             */
/* use_graph!=0 captures the sequence into a hipGraph on first use and replays it.        */
int dlwp_fno_trainer_fwd_bwd(dlwp_fno_trainer* tr, int use_graph, void* stream);

/* ------------------------------------------------------------------------------------ */
/* AFNO2D spectral token mixer (FourCastNet): y = x + irfft2(softshrink(MLP_blockdiag(    */
/* rfft2(x)))) on channels-last x [B,H,W,C].  Replaces AFNO2D.forward                     */
/* nsbench/models/fourcastnet/fourcastnet.py:77-126 (dlwpbench twin :78-127), including   */
/* its kept-mode window computed from H only (:92-93).  Parameter layouts are the         */
/* reference's: w1,w2 [2,nb,bs,bs] (re/im), b1,b2 [2,nb,bs]; hidden_size_factor = 1.      */
/* xsave: caller buffer of dlwp_afno2d_save_elems() floats holding the kept spectrum for   */
/* the backward pass.  Round-1 limits: block size <= 16, H*kept_cols*bs <= 10240 (16x16,   */
/* 32x64 grids); larger grids return DLWP_E_UNSUPPORTED.                                   */
long long dlwp_afno2d_save_elems(int B, int H, int W, int C, int nb, float hard_thresholding_fraction);
int dlwp_afno2d_fwd(const float* x, const float* w1, const float* b1, const float* w2,
                    const float* b2, float* y, float* xsave, int B, int H, int W, int C, int nb,
                    float sparsity_threshold, float hard_thresholding_fraction, void* stream);
/* The same with the block's outer skip folded in (Block.forward, fourcastnet.py:156-160:   */
/* `x = filter(norm1(x)); x = x + residual`): y = AFNO2D(x) + residual, residual [B,H,W,C]   */
/* nullable.  Its gradient is the upstream gradient itself; dlwp_afno2d_bwd is unchanged.    */
int dlwp_afno2d_fwd_res(const float* x, const float* residual, const float* w1, const float* b1,
                        const float* w2, const float* b2, float* y, float* xsave, int B, int H,
                        int W, int C, int nb, float sparsity_threshold,
                        float hard_thresholding_fraction, void* stream);
/* gx = d loss/d x (includes the residual path); gw1,gb1,gw2,gb2 are ACCUMULATED into.     */
int dlwp_afno2d_bwd(const float* gy, const float* xsave, const float* w1, const float* b1,
                    const float* w2, const float* b2, float* gx, float* gw1, float* gb1,
                    float* gw2, float* gb2, int B, int H, int W, int C, int nb,
                    float sparsity_threshold, float hard_thresholding_fraction, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Fused window attention core (Swin W-MSA / SW-MSA and Pangu EarthAttention3D): out =     */
/* softmax(scale q k^T + bias + mask) v without materialising the [windows,heads,N,N]      */
/* scores.  Replaces the middle of WindowAttention.forward nsbench/models/swintransformer/  */
/* swin_transformer.py:134-152 (dlwpbench :133-151) and of EarthAttention3D.forward         */
/* dlwpbench/models/panguweather/panguweather.py:186-208; qkv / proj Linear stay outside.   */
/*   qkv    : [B_, N, 3, heads, d]  (the reference's reshape of the qkv Linear output)      */
/*   bias_table : [TB, ntypes, heads]; the bias of (query q, key k) is                       */
/*            table[ia[q] + ib[k]][window % ntypes][head]  (ia, ib: int32 [N]).  Swin:        */
/*            ntypes = 1, ia = y(2Ww-1)+x, ib = (Wh-1-y)(2Ww-1)+(Ww-1-x); Pangu: see          */
/*            utils/earth_position_index.py:4-45 (index additive in query and key).            */
/*   labels : [nW, N] int32 region labels of the shifted-window mask or NULL; the mask       */
/*            value is -100 where labels differ (swin_transformer.py:377-395)                */
/*   out    : [B_, N, heads*d];  lse : [B_, heads, N] (saved for backward)                   */
/* B_ = batch*nW with the window index fastest.  head_dim d <= 64.                           */
int dlwp_window_attn_fwd(const float* qkv, const float* bias_table, const int* ia, const int* ib,
                         const int* labels, float* out, float* lse, int B_, int nW, int N, int TB,
                         int ntypes, int heads, int d, float scale, void* stream);
/* gqkv is written; gbias_table is ACCUMULATED into; dsum: scratch [B_, heads, N].           */
/* slab: optional scratch of dlwp_window_attn_bwd_slab_floats() floats -- the workgroups then */
/* store their bias-gradient partials there and a fold kernel sums them (one atomic per       */
/* FOLD chunk instead of TB atomics per workgroup); NULL: direct atomics.                     */
/* Earth-specific tables (Pangu: [TB][window types][heads], a head's slice strided by types*heads floats) make   */
/* every workgroup gather its slice one cache line per entry.  pack_table writes the transposed copy               */
/* packed[type][head][TB] once per call; the *_packed entries read contiguous slices from it (packed_table NULL:    */
/* the strided gather, as in the plain entries).  The gradient still goes to the reference-layout gbias_table.      */
int dlwp_window_attn_pack_table(const float* bias_table, float* packed, int TB, int ntypes, int heads,
                                void* stream);
int dlwp_window_attn_fwd_packed(const float* qkv, const float* bias_table, const float* packed_table,
                                const int* ia, const int* ib, const int* labels, float* out, float* lse,
                                int B_, int nW, int N, int TB, int ntypes, int heads, int d, float scale,
                                void* stream);
int dlwp_window_attn_bwd_packed(const float* qkv, const float* bias_table, const float* packed_table,
                                const int* ia, const int* ib, const int* labels, const float* out,
                                const float* lse, const float* gout, float* gqkv, float* gbias_table,
                                float* dsum, float* slab, int B_, int nW, int N, int TB, int ntypes,
                                int heads, int d, float scale, void* stream);
/* Windows whose tokens outside [q_lo, q_hi) are padding that the caller crops (Pangu's pressure-level pad,           */
/* src/dlwpbench/models/panguweather/panguweather.py:283-317: one plane of every (2,7,7) window): the padded tokens  */
/* stay keys / values, their own rows are skipped where the kernel family can (out / lse rows outside the range are  */
/* then unwritten; gout rows outside it are taken as zero; their gqkv query part is written as zero).                */
int dlwp_window_attn_fwd_qrange(const float* qkv, const float* bias_table, const float* packed_table,
                                const int* ia, const int* ib, const int* labels, float* out, float* lse,
                                int B_, int nW, int N, int TB, int ntypes, int heads, int d, float scale,
                                int q_lo, int q_hi, void* stream);
int dlwp_window_attn_bwd_qrange(const float* qkv, const float* bias_table, const float* packed_table,
                                const int* ia, const int* ib, const int* labels, const float* out,
                                const float* lse, const float* gout, float* gqkv, float* gbias_table,
                                float* dsum, float* slab, int B_, int nW, int N, int TB, int ntypes,
                                int heads, int d, float scale, int q_lo, int q_hi, void* stream);

/* bf16 tensors in the window layout (round 6; reference: WindowAttention.forward, swin_transformer.py:123-155, under torch.autocast      */
/* the qkv projection's output, the attention output and their gradients are bf16 tensors there too): qkv [B_, N, 3, heads, d], out and */
/* gout [B_, N, heads, d] and gqkv are bf16 arrays; lse, the bias table and its gradient stay fp32.  Whole query range only.  Supported */
/* where dlwp_window_attn_io_bf16_supported(N, d, TB, B_ * heads) returns 1 (windows of at most 64 tokens, head_dim % 4 == 0, bf16      */
/* matrix mode); otherwise DLWP_E_UNSUPPORTED.                                                                                           */
int dlwp_window_attn_io_bf16_supported(int N, int d, int TB, long long pairs);
int dlwp_window_attn_fwd_bf16(const void* qkv, const float* bias_table, const float* packed_table, const int* ia, const int* ib,
                              const int* labels, void* out, float* lse, int B_, int nW, int N, int TB, int ntypes, int heads, int d,
                              float scale, void* stream);
int dlwp_window_attn_bwd_bf16(const void* qkv, const float* bias_table, const float* packed_table, const int* ia, const int* ib,
                              const int* labels, const void* out, const float* lse, const void* gout, void* gqkv, float* gbias_table,
                              int B_, int nW, int N, int TB, int ntypes, int heads, int d, float scale, void* stream);
long long dlwp_window_attn_bwd_slab_floats(int B_, int N, int heads, int TB);
/* Debug: the accounting name(s), ';'-separated, of the attention kernel(s) a call of this shape would launch under the precision   */
/* mode and tuning knobs in force (the slab fold and the table packing, which depend on the caller's buffers, are not listed), or  */
/* DLWP_E_UNSUPPORTED with the refusal the entry would report.  direction: 0 forward, 1 backward.  layout: 0 = fp32 arrays in the  */
/* window layout (_fwd / _bwd, _packed, _qrange); bit 0: the _tokens entries, bit 1: with fill != NULL, bit 2: bf16 tensors (alone: */
/* _fwd_bf16 / _bwd_bf16).  pairs = B_ * heads.  Reads host state only: works without a device.                                     */
int dlwp_window_attn_route_name(int direction, int layout, int N, int d, int TB, long long pairs, int q_lo, int q_hi, char* buf,
                                int n);
/* Backward of  reverse(crop) . attention . partition(pad with `fill`)  in ONE launch, for a block whose qkv projection ran */
/* on the real tokens (EarthSpecificBlock.forward, src/dlwpbench/models/panguweather/panguweather.py:283-317: ZeroPad3d ->   */
/* roll -> window_partition -> attention -> window_reverse -> roll -> crop3d; SwinTransformerBlock likewise).  The upstream   */
/* gradient and the qkv gradient stay in the UNPARTITIONED token layout:                                                     */
/*   gout_tokens [B][Ltok][heads*d]   window position n of window w (of nW per sample) reads token dst_map[w*N + n]          */
/*                                     (-1: the position is cropped, zero upstream gradient);                                */
/*   gqkv_tokens [B][Ltok][3*heads*d] written at token src_map[w*N + n]; positions with src_map < 0 are padding that held    */
/*                                     `fill` (the qkv bias): their gradient is summed into gfill [3*heads*d] (ACCUMULATED).  */
/* Both maps are int32 [nW][N], the same for every sample; src_map must hit every token exactly once (constant padding,      */
/* no circular copies).  fill == NULL: qkv / out are the window-layout tensors the forward produced                          */
/* (dlwp_window_attn_fwd_qrange on a gathered qkv).  fill != NULL ([3*heads*d], the qkv bias): the OPERANDS are in the token   */
/* layout too -- qkv [B][Ltok][3*heads*d] read through src_map (padded positions hold fill), out [B][Ltok][heads*d] through   */
/* dst_map, as dlwp_window_attn_fwd_tokens left them; lse stays [B_][heads][N].                                              */
/* Replaces the gather of gout, dlwp_window_attn_bwd_qrange, dlwp_window_scatter and dlwp_window_pad_colsum of that chain.   */
/* Needs the bf16 matrix mode, N <= 128, d <= 32, d % 4 == 0 (dlwp_window_attn_bwd_tokens_supported); otherwise              */
/* DLWP_E_UNSUPPORTED and nothing is launched.                                                                               */
int dlwp_window_attn_bwd_tokens_supported(int N, int d, int TB);
int dlwp_window_attn_bwd_tokens(const float* qkv, const float* fill, const float* bias_table, const float* packed_table,
                                const int* ia, const int* ib, const int* labels, const float* out, const float* lse,
                                const float* gout_tokens, const int* dst_map, const int* src_map, float* gqkv_tokens,
                                float* gfill, float* gbias_table, int B_, int nW, int N, int Ltok, int TB, int ntypes,
                                int heads, int d, float scale, int q_lo, int q_hi, int io_bf16, void* stream);
/* io_bf16 != 0 (both entries; needs fill != NULL): the four token-layout tensors -- qkv, out, gout_tokens, gqkv_tokens -- are  */
/* bf16 arrays behind the float pointers (the qkv projection wrote bf16, the output projection reads bf16, and their backward   */
/* GEMMs take the gradients as bf16 operands without a cast pass); fill / gfill / tables / lse stay fp32.                       */
/* The forward of the same chain in one launch: attention over the windows of a token-layout qkv tensor (no gathered copy),   */
/* output rows written to the tokens dst_map names (positions it drops are computed only as keys / values).  Same shape       */
/* family as the wave-per-window kernels: N <= 128, d <= 32, d % 4 == 0, at least 2048 (window, head) pairs, bf16 matrix mode  */
/* (dlwp_window_attn_fwd_tokens_supported); otherwise DLWP_E_UNSUPPORTED.  lse rows outside the computed query chunks are     */
/* written as zero (the backward entry stages every row's statistic); out rows are written exactly once per token.            */
int dlwp_window_attn_fwd_tokens_supported(int N, int d, long long pairs);
int dlwp_window_attn_fwd_tokens(const float* qkv_tokens, const float* fill, const float* bias_table, const float* packed_table,
                                const int* ia, const int* ib, const int* labels, const int* src_map, const int* dst_map,
                                float* out_tokens, float* lse, int B_, int nW, int N, int Ltok, int TB, int ntypes, int heads,
                                int d, float scale, int q_lo, int q_hi, int io_bf16, void* stream);
int dlwp_window_attn_bwd(const float* qkv, const float* bias_table, const int* ia, const int* ib,
                         const int* labels, const float* out, const float* lse, const float* gout,
                         float* gqkv, float* gbias_table, float* dsum, float* slab, int B_, int nW,
                         int N, int TB, int ntypes, int heads, int d, float scale, void* stream);

/* Head dimensions above 64 (deep stages of the nsbench Swin U-Net: the shipped swintransformer.yaml reaches    */
/* head_dim 192 on its 4 x 4 token map): the host runs q k^T and p v as dlwp_gemm_batched around these two row      */
/* kernels, with the scores s / p [B_, heads, N, N] in HBM (N <= 1024).                                              */
/*   fwd (in place): p = softmax(scale s + table[ia[q] + ib[k]][window % ntypes][head] + mask)                      */
/*   bwd (in place): ds = p (dp - rowsum(p dp)); gbias_table += ds; dp <- scale ds                                  */
int dlwp_window_softmax_fwd(float* s, const float* bias_table, const int* ia, const int* ib, const int* labels,
                            int B_, int nW, int N, int ntypes, int heads, float scale, void* stream);
int dlwp_window_softmax_bwd(const float* p, float* dp, float* gbias_table, const int* ia, const int* ib, int B_,
                            int nW, int N, int ntypes, int heads, float scale, void* stream);

/* ------------------------------------------------------------------------------------ */
/* rFFT2 / irFFT2 of real fields of ANY size, butterflies staged in LDS (mixed-radix Stockham */
/* per axis: radices 4, 2, 3, 5, 7 and whatever prime is left, e.g. 721 = 7 x 103).  Replaces  */
/* torch.fft.rfft2 / irfft2(x, dim=(1, 2), norm="ortho") on channels-last [B, H, W, C] tensors  */
/* (AFNO2D.forward, nsbench/models/fourcastnet/fourcastnet.py:84,123; dlwpbench twin :85,124)   */
/* and rfftn / irfftn(norm="forward") over the last dims of [B, C, H, W] (neuralop SpectralConv, */
/* App. A-1).  layout 0: x [B][H][W][C] <-> X [B][H][W/2+1][C][2] (C even);                      */
/* layout 1: x [B][C][H][W] <-> X [B][C][H][W/2+1][2].  norm: 0 "backward", 1 "ortho",           */
/* 2 "forward" (torch.fft's meaning).  adjoint != 0 selects the transposed transform of the       */
/* OTHER direction with the same norm, i.e. the backward pass:                  */
/*   dlwp_irfft2(adjoint=1): gX (spectrum) -> gx = rfft2^H gX   (interior bins weigh one half)     */
/*   dlwp_rfft2 (adjoint=1): gx (field)    -> gX = irfft2^H gx  (interior bins weigh two)          */
/* DC / Nyquist imaginary parts are ignored by irfft2, as in torch.  work: scratch of X's size.    */
typedef struct dlwp_fft_plan dlwp_fft_plan;
int dlwp_fft_plan_create(int H, int W, dlwp_fft_plan** out);
void dlwp_fft_plan_destroy(dlwp_fft_plan* plan);
int dlwp_rfft2(const dlwp_fft_plan* plan, const float* x, float* X, int B, int C, int layout, int norm,
               int adjoint, void* stream);
int dlwp_irfft2(const dlwp_fft_plan* plan, const float* X, float* x, float* work, int B, int C, int layout,
                int norm, int adjoint, void* stream);
/* The channels-last pair with a WINDOW of the half spectrum as two planes,                          */
/* X [2 (re | im)][B][r1 - r0][c1][C] = rows r0 <= kh < r1, columns kw < c1 of rfft2's [B][H][W/2+1][C]: */
/* the kept modes AFNO2D's block-diagonal complex MLP works on (fourcastnet.py:85-124: rfft2, the slice */
/* x[:, total_modes-kept_modes:total_modes+kept_modes, :kept_modes], irfft2 of the zero-initialised     */
/* result), in the planar layout of the real batched GEMMs that replace the complex einsums -- no copy  */
/* or zero fill between transform and products.  irfft2_planar reads zeros outside the window; adjoint  */
/* as above.  work: scratch of the FULL half spectrum's size (2 B H (W/2+1) C floats).                  */
/* bs > 0 (a divisor of C): block-planar instead, X [B][r1 - r0][c1][C / bs][2 (re | im)][bs] -- with   */
/* dlwp_afno_wq_expand_bp's weights the complex block MLP of a layer is ONE real batched GEMM.          */
int dlwp_rfft2_planar(const dlwp_fft_plan* plan, const float* x, float* X, float* work, int B, int C, int r0, int r1,
                      int c1, int bs, int norm, int adjoint, void* stream);
/* residual (field-shaped [B][H][W][C], or NULL) is added to irfft2_planar's output: AFNO2D's `x + bias` skip    */
/* (fourcastnet.py:126) in the forward pass, the gradient arriving along that skip in the backward pass.      */
/* dlwp_rfft2_planar whose store folds in the derivative of a soft-shrink: a stored component is zeroed where the same   */
/* element of `mask` (X's layout: the saved pre-activation of AFNO2D's second block layer, fourcastnet.py:117-121          */
/* F.softshrink) has magnitude <= lam -- the backward transform of the filter then delivers the gradient of that           */
/* pre-activation directly (no dlwp_act_bwd pass).  mask NULL: dlwp_rfft2_planar.                                          */
int dlwp_rfft2_planar_masked(const dlwp_fft_plan* plan, const float* x, float* X, float* work, const float* mask, float lam,
                             int B, int C, int r0, int r1, int c1, int bs, int norm, int adjoint, void* stream);
/* The planar pair with the spectrum window as a bf16 array (flags = 1; bf16 storage of the AFNO block MLP's operands:  */
/* the reference's einsums run under bf16 autocast, fourcastnet.py:100-121): dlwp_rfft2_planar_ex writes X (and reads    */
/* the mask) as bf16, dlwp_irfft2_planar_ex reads X as bf16; fields, work and residuals stay fp32.  flags = 0: the      */
/* entries above.                                                                                                        */
int dlwp_rfft2_planar_ex(const dlwp_fft_plan* plan, const float* x, void* X, float* work, const void* mask, float lam, int B,
                         int C, int r0, int r1, int c1, int bs, int norm, int adjoint, int flags, void* stream);
int dlwp_irfft2_planar_ex(const dlwp_fft_plan* plan, const void* X, float* x, float* work, const float* residual,
                          const float* residual2, int B, int C, int r0, int r1, int c1, int bs, int norm, int adjoint,
                          int flags, void* stream);
int dlwp_irfft2_planar(const dlwp_fft_plan* plan, const float* X, float* x, float* work, const float* residual, int B,
                       int C, int r0, int r1, int c1, int bs, int norm, int adjoint, void* stream);
/* ... with a second field added in the same store (the AFNO block's outer skip around the filter,                 */
/* fourcastnet.py:156-165 `x = self.filter(x); if self.double_skip: x = x + residual`); residual2 needs residual.   */
int dlwp_irfft2_planar2(const dlwp_fft_plan* plan, const float* X, float* x, float* work, const float* residual,
                        const float* residual2, int B, int C, int r0, int r1, int c1, int bs, int norm, int adjoint,
                        void* stream);

/* General-grid AFNO2D (grids whose block spectrum does not fit LDS): the transforms run as     */
/* dlwp_gemm_batched against DFT tables and the per-mode block MLP as batched GEMMs over the     */
/* channel blocks, on the real image of the complex block weights w [2][nb][bs_in][bs_out]       */
/* (fourcastnet.py:70-75): wq[ri][ro][blk][i][o] = {Wr, Wi; -Wi, Wr}.  fold ACCUMULATES the     */
/* complex gradient from a wq-shaped gradient.                                                   */
int dlwp_afno_wq_expand(const float* w, float* wq, int nb, int bs_in, int bs_out, void* stream);
int dlwp_afno_wq_fold(const float* gq, float* gw, int nb, int bs_in, int bs_out, void* stream);
/* Block-planar form (tokens [T][blk][re | im][bs], dlwp_rfft2_planar with bs > 0): wq [blk][ri][i][ro][o], one  */
/* real 2 bs_in x 2 bs_out matrix per channel block, and the bias b [2][nb][bs_out] reordered to bq [blk][ro][o]; */
/* fold ACCUMULATES both gradients (gw, gb in the reference's parameter layouts, fourcastnet.py:70-75).           */
int dlwp_afno_wq_expand_bp(const float* w, const float* b, float* wq, float* bq, int nb, int bs_in, int bs_out, void* stream);
int dlwp_afno_wq_fold_bp(const float* gq, const float* gbq, float* gw, float* gb, int nb, int bs_in, int bs_out,
                         void* stream);

/* Window partition / reverse of shifted-window attention as one gather each (the reference  */
/* runs pad, roll, partition / reverse, roll, crop as separate full-tensor copies:             */
/* nsbench swin_transformer.py:213-250, dlwpbench panguweather.py:283-317).                    */
/* tokens x [B][D0][D1][D2][C] <-> windows [B*nW][w0*w1*w2][C]; all arrays have 3 entries       */
/* (use 1 for unused leading axes): dims D, padded sizes P (multiples of the window), front     */
/* pads, roll shifts s (rolled[i] = padded[(i + s) mod P], i.e. torch.roll by -s), window sizes, */
/* strides of the window-grid index inside a sample's nW windows, circular (1) or zero (0)       */
/* padding per axis.  scatter with sum_copies != 0 sums every padded copy of a token (adjoint    */
/* of a circularly padded gather).  C must be a multiple of 4.                                   */
int dlwp_window_gather(const float* x, float* windows, int B, int C, const int* dims,
                       const int* padded, const int* front, const int* shift, const int* window,
                       const long long* wstride, const int* circular, void* stream);
/* dlwp_window_gather on a tensor that a token-wise Linear layer has already produced: the padded positions hold  */
/* `fill` [C] (that layer's bias; NULL: zero) -- "pad, then Linear on every window token" == "Linear on the real    */
/* tokens, then pad with the bias" (reference: the qkv projection of EarthAttention3D on the zero-padded windows,   */
/* panguweather.py:283-292,176), so the GEMM runs on the real tokens only.  dlwp_window_pad_colsum is the fill's    */
/* adjoint: gfill[c] += sum over the padded positions of g_windows[..][c] for c >= c_lo (a multiple of 4; lets the   */
/* caller skip channels whose padded rows are known to be zero).                                                   */
int dlwp_window_gather_fill(const float* x, const float* fill, float* windows, int B, int C, const int* dims,
                            const int* padded, const int* front, const int* shift, const int* window,
                            const long long* wstride, const int* circular, void* stream);
int dlwp_window_pad_colsum(const float* g_windows, float* gfill, int B, int C, const int* dims,
                           const int* padded, const int* front, const int* shift, const int* window,
                           const long long* wstride, const int* circular, int c_lo, void* stream);
int dlwp_window_scatter(const float* windows, float* x, int B, int C, const int* dims,
                        const int* padded, const int* front, const int* shift, const int* window,
                        const long long* wstride, const int* circular, int sum_copies,
                        void* stream);
/* dlwp_window_scatter with the block's skip connection folded in: x = residual + reverse(windows)  */
/* (`x = shortcut + drop_path(x)` after window_reverse / roll / crop, swin_transformer.py:250-255 and */
/* panguweather.py:317-319); residual [B][D0*D1*D2][C] nullable.                                      */
int dlwp_window_scatter_add(const float* windows, const float* residual, float* x, int B, int C,
                            const int* dims, const int* padded, const int* front, const int* shift,
                            const int* window, const long long* wstride, const int* circular,
                            int sum_copies, void* stream);
/* Round 5: the gather / scatter pair on bf16 arrays and with the branch's stochastic depth folded in.            */
/* dlwp_window_gather_ex: dlwp_window_gather_fill (fill nullable) with flags bit 0 = x is a bf16 array, bit 1 =     */
/* windows is one, and scale [B] (nullable): the gathered values of sample b are multiplied by scale[b].            */
/* dlwp_window_scatter_ex: x[b] = residual[b] + scale[b] * reverse(windows)[b] (`x = shortcut + drop_path(x)` after */
/* window_reverse, swin_transformer.py:250-256): flags bit 0 = windows is a bf16 array, bit 1 = x is one; residual  */
/* (fp32, nullable) and scale [B] (fp32, nullable).  Each is the other's adjoint with the same scale.               */
int dlwp_window_gather_ex(const void* x, const float* fill, const float* scale, void* windows, int B, int C,
                          const int* dims, const int* padded, const int* front, const int* shift,
                          const int* window, const long long* wstride, const int* circular, int flags,
                          void* stream);
int dlwp_window_scatter_ex(const void* windows, const float* residual, const float* scale, void* x, int B, int C,
                           const int* dims, const int* padded, const int* front, const int* shift,
                           const int* window, const long long* wstride, const int* circular,
                           int sum_copies, int flags, void* stream);
/* Epilogue of a transposed convolution with kernel == stride on channels-last tokens (the Swin U-decoder's          */
/* nn.ConvTranspose2d(k, stride k) + GELU, src/nsbench/models/swintransformer/swin_transformer.py:580-588, dlwpbench  */
/* twin): y [B*H*W][O*kh*kw] is the GEMM x . W[Cin][O*kh*kw] in the weight's own layout; forward: dst[b][h kh+i][w kw+j] */
/* [coff+o] = act(y + bias[o]) with pixel pitch ctot (dst may be the concat buffer of the next level), act 0 none / 1     */
/* GELU; backward != 0: dst = gy [B*H*W][O*kh*kw] = gout * act'(y + bias), gbias[o] += its sums (nullable).               */
int dlwp_upconv_shuffle(const float* y, const float* bias, const float* gout, float* dst, float* gbias,
                        int B, int H, int W, int O, int kh, int kw, int ctot, int coff, int act,
                        int backward, void* stream);
/* Patch merging gather (PatchMerging.forward, src/nsbench/models/swintransformer/swin_transformer.py:291-312 */
/* and the dlwpbench twin): tokens x [B][H][W][C] -> [B][ceil(H/2)][ceil(W/2)][4C] with channel blocks in the    */
/* reference's concat order (0,0), (1,0), (0,1), (1,1) and zeros beyond an odd H / W (its constant pad).        */
/* backward != 0 runs the adjoint: src is the gradient [B][H2][W2][4C], dst the gradient [B][H][W][C].          */
int dlwp_patch_merge(const float* src, float* dst, int B, int H, int W, int C, int backward, void* stream);
/* One lead time of an autoregressive rollout on its sliding input window (csrc/rollout_ops.hip; the reference  */
/* rebuilds the window with stack + cat + add on every step: src/nsbench/models/fourcastnet/fourcastnet.py:     */
/* 262-300, swintransformer/swin_transformer.py:597-640, src/dlwpbench/models/unet/unet.py:64-111):              */
/*   next[b][j] = win[b][j+1] (j < ctx-1);  next[b][ctx-1] = out[b] = win[b][ctx-1] + delta[b].                  */
/* win: [B][ctx][frame] with a batch stride in floats (a slice of the data tensor qualifies); next (nullable:    */
/* last step) [B][ctx][frame]; out [B][frame].  delta_layout 0: delta is [B][frame]; 1: delta holds the patch    */
/* tokens of a linear head, [B][H/ph][W/pw][ph][pw][D] with frame = D*H*W (AFNONet.head output, :296-298).        */
int dlwp_window_advance_fwd(const float* win, long long win_batch_stride, const float* delta, float* next,
                            float* out, int B, int ctx, long long frame, int delta_layout, int D, int H,
                            int W, int ph, int pw, void* stream);
/* Its adjoint, which also sums the gradients that reach the window from its (up to) three readers: g_next from  */
/* the following advance [B][ctx][frame], g_net from the network that read the window (batch stride given: a     */
/* channel slice of a wider input gradient qualifies), g_out from the loss ([B][frame], batch stride given).      */
/* Any of the three may be NULL.  g_win (nullable: the window was data) [B][ctx][frame]; g_delta in delta's layout. */
int dlwp_window_advance_bwd(const float* g_next, const float* g_net, long long net_batch_stride,
                            const float* g_out, long long out_batch_stride, float* g_win, float* g_delta,
                            int B, int ctx, long long frame, int delta_layout, int D, int H, int W, int ph,
                            int pw, void* stream);
/* HEALPix faces <-> the patch tokens of the 3n x 4n canvas (csrc/hpx_canvas.hip; SwinTransformerHPX._faces2rect,  */
/* _prepare_inputs and _reshape_output, src/dlwpbench/models/swintransformer/swin_transformer.py:826-879): face f, */
/* pixel (y, x) sits at canvas row (f / 4) n + y, column (f % 4) n + x.  gather: up to three face tensors, each    */
/* (pointer, batch stride in floats, channels C_k) with a dense [C_k][12][n][n] block per sample (a skipped source */
/* is NULL with 0 channels), -> tok [B][3n/ph][4n/pw][Ctot][ph][pw], Ctot = C0 + C1 + C2 in source order: the rows  */
/* of the patch-embedding GEMM (for patch 1 x 1 the channels-last canvas).  scatter, its adjoint: channels           */
/* [c0, c0 + C) of a tok tensor in that layout -> dense faces [B][C][12][n][n].  Pure data movement, bit-exact.     */
int dlwp_hpx_canvas_gather(const float* src0, long long bs0, int C0, const float* src1, long long bs1, int C1,
                           const float* src2, long long bs2, int C2, float* tok, int B, int n, int ph, int pw,
                           void* stream);
int dlwp_hpx_canvas_scatter(const float* tok, float* faces, int B, int n, int ph, int pw, int Ctot, int c0, int C,
                            void* stream);
/* HEALPix <-> lat-lon remap (csrc/hpx_remap.hip; HEALPixRemap.ll2hpx / hpx2ll, data/processing/healpix_mapping.py:328-399, and   */
/* the projection to lat-lon in front of compute_metrics, scripts/evaluate.py:71-109, 215-220).  A remap is a table of 4 source   */
/* indices and 4 weights per output point (dlwp_benchmark_amd/hpx_geometry.py) applied to `planes` = B T C maps at once.          */
/* PRECONDITION (the kernels cannot check device tables; the Python side checks in numpy before the upload):                      */
/* 0 <= idx[i] < n_in, rowptr[0] = 0 <= rowptr[r] <= rowptr[r + 1], 0 <= col[e] < n_in.  idx and w are 16-byte aligned.           */
/*   gather4: dst[p][o] = sum_{k<4} w[4o+k] src[p src_plane_stride + idx[4o+k]], p < planes, o < n_out; dst dense [planes][n_out], */
/*            src_plane_stride >= n_in floats.  Two kernels: LDS-staged plane tiles while a plane fits 72 KiB, else global gathers */
/*            with the taps in registers; the knob REMAP_PATH (0 auto, 1 LDS, 2 direct) forces one, a forced LDS path that does    */
/*            not fit returns DLWP_E_UNSUPPORTED.                                                                                  */
/*   csr    : dst[p][r] (+)= sum_{rowptr[r] <= e < rowptr[r+1]} val[e] src[p][col[e]] in ascending e, no atomics (bit-reproducible): */
/*            the adjoint of gather4 with the transposed table; src dense [planes][n_in], dst dense [planes][n_out] (n_out rows),  */
/*            accumulate != 0 adds to dst.                                                                                         */
int dlwp_remap_gather4(const float* src, long long src_plane_stride, const int* idx, const float* w, float* dst,
                       long long planes, int n_in, int n_out, void* stream);
int dlwp_remap_csr(const float* src, const int* rowptr, const int* col, const float* val, float* dst, long long planes,
                   int n_in, int n_out, int accumulate, void* stream);
/* dlwp_error_moments of fields on the HEALPix mesh scored on a lat-lon grid: out / target [B][G][12][n][n] are interpolated   */
/* through the hpx2ll table idx / w [H W][4] inside the kernel (no lat-lon tensor is written); climatology [B][G][H][W] or NULL */
/* and row_weights [H] or NULL are on lat-lon.  moments [5][G] is ACCUMULATED into, as by dlwp_error_moments.                   */
int dlwp_hpx_error_moments(const float* out_hpx, const float* target_hpx, const float* climatology_ll,
                           const float* row_weights, const int* idx, const float* w, int B, int G, int n, int H, int W,
                           float* moments, void* stream);
/* Long-rollout diagnostics in one read of a chunk of outputs and targets (csrc/rollout_diag.hip; the physical-soundness half of      */
/* compute_metrics, scripts/evaluate.py:548-588, beside its per-lead RMSE / ACC :514-546, and the persistence / climatology forecasts */
/* of scripts/build_baselines.py:23-67).  ONE entry point for both meshes: idx / w == NULL scores lat-lon planes, out / target        */
/* [Bc][Tc][V][H][W]; with the hpx2ll table idx / w [H W][4] (both, 16-byte aligned; 0 <= idx < 12 n^2 is the caller's precondition)  */
/* out / target are [Bc][Tc][V][12][n][n] and are interpolated inside the kernel (no lat-lon tensor is written).                      */
/*   out      : frame (b, t) of variable v starts at out + b out_bstride + t out_tstride + v plane (element strides >= 0, plane = H W  */
/*              or 12 n^2; a time stride of 0 is the persistence forecast, one frame per sample read in place); NULL with clim given: */
/*              the forecast is the climatology.  target is dense.                                                                    */
/*   scale, shift [V] or NULL (identity): physical = x * scale + shift.  row_weights [H] or NULL.                                      */
/*   clim [M][V][H][W] on lat-lon in PHYSICAL units with month [Bc][Tc] (int32, 0 <= month < M: the caller's precondition; the kernel */
/*              clamps), both or neither.                                                                                             */
/*   t_begin  : global index of the chunk's first frame in a rollout of T frames; [w0, w1): a window of global frame indices.         */
/*   moments [Bc][T][V][5] : the five sums of dlwp_error_moments per sample, lead time and variable in physical units; WRITTEN for the */
/*              chunk's frames (columns 2-4 are 0 without clim)                                                                       */
/*   zonal [2][Bc][T][V][H]: the longitude mean of the de-normalised out (0) and target (1); WRITTEN for the chunk's frames           */
/*   wsum [2][Bc][V][H][W] : the sum of the NORMALISED out / target over the chunk's frames inside the window, ACCUMULATED into: the  */
/*              caller zeroes it before the first chunk; the window mean is wsum / (w1 - w0) * scale + shift                           */
/*   ws       : dlwp_rollout_diag_ws_floats(Bc, Tc, V, H, W, hpx) floats of scratch (per-wave moment partials)                         */
/* All sums are taken of the normalised values (the climatology is brought into normalised units per pixel) and scaled afterwards.    */
/* No atomics, one writer per address, a summation order that depends on (H, W, mesh) only: two runs give the same bits, and scoring  */
/* a rollout in time chunks and batch chunks gives the bits of one call (order: csrc/rollout_diag.hip).  HPX planes are staged in LDS */
/* while two planes fit 72 KiB, else gathered from global memory; the knob DIAG_PATH (0 auto, 1 LDS, 2 direct) forces one.  W <= 512.  */
long long dlwp_rollout_diag_ws_floats(int Bc, int Tc, int V, int H, int W, int hpx);
int dlwp_rollout_diag(const float* out, long long out_bstride, long long out_tstride, const float* target,
                      const float* scale, const float* shift, const float* row_weights, const float* clim,
                      const int* month, int M, const int* idx, const float* w, int n, int Bc, int Tc, int V, int H, int W,
                      int t_begin, int T, int w0, int w1, float* moments, float* zonal, float* wsum, float* ws,
                      void* stream);
/* Group means (the monthly climatology of scripts/build_baselines.py:52-62): frames [N][P], group [N] (int32, 0 <= group < G: the    */
/* caller's precondition; other values are skipped) -> mean [G][P], count [G] (int32).  Each frame is read once, added in ascending   */
/* n, no atomics; an empty group gives count 0 and a zero row.  G <= 64.                                                              */
int dlwp_group_mean(const float* frames, const int* group, float* mean, int* count, long long N, long long P, int G,
                    void* stream);
/* Power spectra of forecast and target per lead time (csrc/spectra.hip; the reference has none: tests/spectra_ref.py defines them).     */
/* Sphere: out / target as dlwp_rollout_diag takes them ([Bc][Tc][V][H][W], or [Bc][Tc][V][12][n][n] with the hpx2ll table idx / w,   */
/* analysed on the table's H x W grid; out with free element strides >= 0 or NULL: the targets alone, power[0] and cross are zero).   */
/*   F  [2 M][W] : rows 2 m, 2 m + 1 = (2 pi / W) cos, -(2 pi / W) sin of 2 pi m n / W                                                  */
/*   Wf [M][L][H]: orthonormal associated Legendre functions P~_l^m(cos theta_k) times the quadrature weight of row k                  */
/*              (both built in float64 and rounded once by the caller: the kernel is grid-agnostic).  L <= H <= 256, M <= W / 2,       */
/*              W <= 512 (the Nyquist order is left out).                                                                               */
/*   power [2][Bc][T][V][L]: P_l = (1 / 4 pi) sum_m c_m |a_lm|^2 of out (0) and target (1), c_0 = 1, c_m = 2, in NORMALISED units       */
/*   cross [Bc][T][V][L]   : (1 / 4 pi) sum_m c_m Re(a_lm^out conj a_lm^target)                                                         */
/*   a00   [2][Bc][T][V]   : Re a_00 (a per-variable shift moves degree 0 only: the host applies it there)                              */
/*   ws    : dlwp_sphere_spectra_ws_floats(Bc, Tc, V, H, W, L, M, n) floats (n = 0: lat-lon)                                            */
/* All three are WRITTEN for the chunk's frames t_begin .. t_begin + Tc - 1 of T.  No atomics, one writer per address, a summation      */
/* order that depends on (H, W, L, M, mesh) only: two runs, and time / batch chunks, give the same bits.  No a_lm and no lat-lon tensor */
/* is written to memory.  Knobs: SPEC_MB / SPEC_RB (orders / rows per block), SPEC_HPX (0 auto, 1 LDS-staged planes, 2 direct).          */
long long dlwp_sphere_spectra_ws_floats(int Bc, int Tc, int V, int H, int W, int L, int M, int n);
int dlwp_sphere_spectra(const float* out, long long out_bstride, long long out_tstride, const float* target, const float* F,
                        const float* Wf, const int* idx, const float* w, int n, int Bc, int Tc, int V, int H, int W, int L, int M,
                        int t_begin, int T, float* power, float* cross, float* a00, float* ws, void* stream);
/* Plane: the shell-binned spectrum of doubly periodic fields out / target [Bc][Tc][D][H][W] (out as above), through dlwp_rfft2           */
/* (channels-first, norm "backward"; `plan` made for H x W is the caller's precondition) into ws and one binning pass.  Shell k is the   */
/* CSR list rowptr [K + 1] / entry [nnz] (index into the half spectrum [H][W/2+1], 0 <= entry < H (W/2+1)) / weight [nnz] (c = 1 on the */
/* self-conjugate columns, 2 otherwise), summed in list order:                                                                          */
/*   power [2][Bc][T][D][K]: E(k) = sum c |u|^2 / (H W)^2;  cross [Bc][T][D][K]: sum c Re(u^out conj u^target) / (H W)^2                 */
/*   ws    : dlwp_plane_spectra_ws_floats(Bc, Tc, D, H, W) floats (the half spectra of one chunk)                                        */
long long dlwp_plane_spectra_ws_floats(int Bc, int Tc, int D, int H, int W);
int dlwp_plane_spectra(const dlwp_fft_plan* plan, const float* out, long long out_bstride, long long out_tstride, const float* target,
                       const int* rowptr, const int* entry, const float* weight, int K, int nnz, int Bc, int Tc, int D, int H, int W,
                       int t_begin, int T, float* power, float* cross, float* ws, void* stream);
/* Seeded ensemble forecasts (csrc/ensemble.hip; the reference has none: tests/ens_ref.py defines them).                                */
/* Perturbation: x [B][F] (one sample's input frames: F = frames x V planes of P floats), items [B] int32, sigma [V] in normalised      */
/* units -> out [B][M][F], out[b][m][e] = x[b][e] + sigma[(e / P) % V] z with z from the stream of dlwp_ns_batch / dlwp_wb_batch,       */
/* counter (e >> 2, items[b], m, DLWP_ENS_TAG), key = the two halves of seed: a member depends on (seed, item, member, element) only,   */
/* never on B, on M or on the call.  control != 0: member 0 is a bit-exact copy and draws nothing.  One launch, pure data movement (no   */
/* atomics, no LDS), x is read once.  1 <= M <= DLWP_ENS_MAX_MEMBERS, F a multiple of V P.                                               */
#define DLWP_ENS_TAG 0x656eu /* Philox counter word 3 of dlwp_ens_perturb */
#define DLWP_ENS_MAX_MEMBERS 64
int dlwp_ens_perturb(const float* x, const int* items, const float* sigma, int B, long long F, long long P, int V, int M, int control,
                     unsigned long long seed, float* out, void* stream);
/* Scores of M members against the target in one read of both, per sample, lead time and variable (NORMALISED values: a shift cancels    */
/* in every score, the host applies the scale).                                                                                          */
/*   members  : frame (b, m, t) of variable v starts at members + b bstride + m mstride + t tstride + v H W (element strides >= 0; a     */
/*              stride of 0 is read in place: an expanded view, the persistence forecast).  target dense [Bc][Tc][V][H][W].               */
/*   row_weights [H] or NULL.                                                                                                            */
/*   sums  [Bc][T][V][4]    : sum over pixels of w_h times (mean - y)^2 | sum_i (x_i - mean)^2 / (M - 1) | sum_i |x_i - y| / M |          */
/*              sum_{i<j} |x_i - x_j| / (M (M - 1)); the fair CRPS is column 2 - column 3                                                 */
/*   ranks [Bc][T][V][M + 1]: (int32) the unweighted count of pixels with #{i : x_i < y} = k; a tie counts as not below                  */
/*   ws    : dlwp_ens_diag_ws_floats(Bc, M, Tc, V, H, W) floats (the pixel blocks' partial sums and counts)                              */
/* Both are WRITTEN for the chunk's frames t_begin .. t_begin + Tc - 1 of T.  2 <= M <= DLWP_ENS_MAX_MEMBERS, H W <= 2^21 (721 x 1440   */
/* fits).  Mean and variance in two passes over registers, relative to member 0 (no E[x^2] - mean^2); the pair term is the O(M^2) loop.  */
/* No atomics, one writer per address, a summation order that depends on (H, W, M) only: two runs, and time / batch chunks, give the     */
/* same bits.  Knob: ENS_BUCKET (0 auto, or 8 / 16 / 32 / 64 members held per thread).                                                    */
long long dlwp_ens_diag_ws_floats(int Bc, int M, int Tc, int V, int H, int W);
int dlwp_ens_diag(const float* members, long long bstride, long long mstride, long long tstride, const float* target,
                  const float* row_weights, int Bc, int M, int Tc, int V, int H, int W, int t_begin, int T, float* sums, int* ranks,
                  float* ws, void* stream);
/* The CRPS of M members as a training loss, with its gradient from the same launch (csrc/ensemble.hip; tests/crps_ref.py defines it).  */
/* Per pixel, with lambda = pair_coeff:  l = (1 / M) sum_i |x_i - y| - lambda / (M (M - 1)) sum_{i<j} |x_i - x_j|  (lambda = 1: the     */
/* fair CRPS, columns 2 - 3 of dlwp_ens_diag; lambda = (M - 1) / M: the ensemble estimator), and                                         */
/*   loss = (1 / N) sum_{b,t,v,h,w} r_h c_v l,  N = B T V H W;  row_weights [H] (r) and var_weights [V] (c) may be NULL (all ones)       */
/*   grad[b][m][t][v][h][w] = (r_h c_v / N) (sgn(x_m - y) / M - lambda / (M (M - 1)) (#{j : x_j < x_m} - #{j : x_j > x_m})),             */
/*   sgn(0) = 0 and a tie x_i == x_j contributes nothing (torch's sub-gradient of abs); dense, WRITTEN; NULL: the loss alone.            */
/*   members as dlwp_ens_diag (element strides >= 0), target dense [B][T][V][H][W], loss_out one float, WRITTEN.                         */
/*   ws    : dlwp_crps_loss_ws_floats(B, M, T, V, H, W) floats (one partial per pixel block)                                             */
/* 2 <= M <= DLWP_ENS_MAX_MEMBERS, H W <= 2^21, 0 <= pair_coeff <= 1.  Two launches, no atomics, one writer per address, a summation     */
/* order that depends on the shape only: two calls give the same bits of the loss and of the gradient.  Knob: ENS_BUCKET.                */
long long dlwp_crps_loss_ws_floats(int B, int M, int T, int V, int H, int W);
int dlwp_crps_loss_fwd_bwd(const float* members, long long bstride, long long mstride, long long tstride, const float* target,
                           const float* row_weights, const float* var_weights, int B, int M, int T, int V, int H, int W, float pair_coeff,
                           float* loss_out, float* grad, float* ws, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Token-level building blocks of the AFNO / Swin / Pangu blocks (nn.Linear, nn.LayerNorm, */
/* nn.GELU call sites: nsbench/models/fourcastnet/fourcastnet.py:44-46,213,233;             */
/* nsbench/models/swintransformer/swin_transformer.py:35-39,131,153,187,194,274).           */
/* C[M,N] (+)= epilogue(op(A)[M,K] . op(B)[K,N]); row-major with leading dimensions;         */
/* epilogue: + bias[n], optional store of the pre-activation, act (0 none, 1 GELU),          */
/* + residual[m,n] (same layout as C); accumulate != 0 adds into C.  rowsum (optional, [M]): */
/* rowsum[m] += sum_k op(A)[m,k] -- the bias gradient of a Linear layer comes out of the      */
/* weight-gradient product gW = gy^T x for free.  Reductions with few output tiles are split  */
/* along K across workgroups and combined with float atomics (summation order not fixed).     */
int dlwp_gemm(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb,
              int ldc, int transA, int transB, const float* bias, int act, float* preact,
              const float* residual, int accumulate, float* rowsum, void* stream);
/* Operand precision of dlwp_gemm / dlwp_gemm_batched, process-wide: 0 (default) = exact fp32 */
/* MFMA; 1 = operands rounded to bf16 in LDS, v_mfma_f32_16x16x32_bf16, fp32 accumulation --   */
/* the arithmetic of the reference's bf16-autocast runs (BASELINE C3-C5).  HBM tensors stay     */
/* fp32 either way.                                                                             */
int dlwp_set_gemm_precision(int mode);
int dlwp_get_gemm_precision(void);
/* 256 x 256 x 64 tiles in two wave groups half a phase apart (bf16 arrays, y = x W^T): -1 never, 0 by shape (K >= 4096 and at    */
/* least 512 tiles: one workgroup per CU leaves its prologue / epilogue uncovered), 1 wherever the kernel applies (measurement).   */
int dlwp_set_gemm_tile256(int mode);
/* Weight gradients of a token MLP's layers in ONE launch: gw_i [N][K] (+)= g_i^T x_i with g_i [T][N] (the gradient of  */
/* the layer's output), x_i [T][K] (its input), gb_i [N] += column sums of g_i (NULL: none) -- what                        */
/* dlwp_gemm_mixed(transA = 1, rowsum = gb) computes per layer (torch.nn.Linear backward in Mlp / SFNO block tails,      */
/* fourcastnet.py:50-56).  Operands fp32 or bf16 arrays (g_bf16 / x_bf16).  Up to three products are grouped;             */
/* otherwise (or when an operand is not 16-byte aligned) they run one launch each.                                      */
typedef struct dlwp_wgrad_desc {
    const void* g;
    const void* x;
    float* gw;
    float* gb;
    int T, N, K;
    int g_bf16, x_bf16, accumulate;
} dlwp_wgrad_desc;
int dlwp_weight_grad_group(const dlwp_wgrad_desc* products, int n, void* stream);
/* The same gradients for a layer applied SEVERAL times with the same weights (the lead times of a rollout,                 */
/* src/dlwpbench/models/fno/fno.py:217-259): gW += sum_s g_s^T x_s and gb += sum_s sum_t g_s[t] as ONE product over the            */
/* concatenated token axis, up to DLWP_WGRAD_MAX_PRODUCTS layers per call (csrc/wgrad_multi.hip).  Every segment is T tokens;       */
/* g_s [T][N], x_s [T][K] bf16 arrays (16-byte aligned, N and K multiples of 8), gw [N][K] and gb [N] fp32, accumulated into.       */
/* The K slices go to the CALLER's workspace (dlwp_wgrad_segments_workspace_bytes) and are added in slice order by a second        */
/* launch: no allocation, no synchronisation, bit-reproducible weight gradients.                                                   */
#define DLWP_WGRAD_MAX_PRODUCTS 6
#define DLWP_WGRAD_MAX_SEGMENTS 8
typedef struct dlwp_wgrad_seg_product {
    const void* g[DLWP_WGRAD_MAX_SEGMENTS];
    const void* x[DLWP_WGRAD_MAX_SEGMENTS];
    float* gw;
    float* gb;                              /* nullable */
    int N, K;
    int overwrite;                          /* != 0: gw = the sum (no read of its old contents); gb is always accumulated into */
} dlwp_wgrad_seg_product;
size_t dlwp_wgrad_segments_workspace_bytes(const dlwp_wgrad_seg_product* products, int nprod, int nseg, int T);
int dlwp_wgrad_segments(const dlwp_wgrad_seg_product* products, int nprod, int nseg, int T, void* workspace,
                        size_t workspace_bytes, void* stream);
/* Any INDEPENDENT small products: between _begin and _end, the dlwp_gemm* entries park products that fit the generic 64 x 64 kernel   */
/* and are small (<= 16384 deep, latency-bound by themselves); _end launches up to three of them as one grid.  Everything else      */
/* launches at once.  Used around the two gradient products of a Linear layer's backward pass (gx = g W and gW = g^T x read the     */
/* same g and do not depend on each other).  One group per HOST THREAD (thread-local queue); not reentrant.  Contract: between       */
/* _begin and _end the caller issues no kernel that depends on a parked product's output, and keeps every operand of a parked        */
/* product alive and unmodified until _end returns (the launches happen there).                                                      */
int dlwp_gemm_group_begin(void);
int dlwp_gemm_group_end(void* stream);
/* Debug: the accounting name(s), ';'-separated, of the kernel(s) a GEMM call would launch under the precision mode, the tile256     */
/* mode and the tuning knobs in force (gemm_slab_reduce_kernel where the K slices go to a slab, which is taken to be available; a    */
/* product the open queue would park and a weight-gradient group member name their group kernel), then '|' and the plan:             */
/* "splits= kchunk= xcd=" (the entry's split-K: C is zeroed first when zero=1), "kernel_splits= kernel_kchunk= kernel_xcd=" (what   */
/* the kernel runs with), "grid=x,z block= lds=" (bytes).  entry: 0 dlwp_gemm / _mixed / _rowscale, 1 dlwp_gemm_batched*, 2 the      */
/* channels-first internal entry, 3 a member of dlwp_weight_grad_group (per_product = its share of the group's workgroup slots, M =  */
/* desc.N, N = desc.K, K = desc.T, transA = 1).  nbatch = nb1 * nb2; strides: NULL or {sA1, sA2, sB1, sB2, sC1, sC2, sR1, sR2,       */
/* sBi1, sBi2}; addr: the addresses of {A, B, C, bias, preact, residual} as integers (0 = absent; only their alignment is read,      */
/* nothing is dereferenced); flags: 1 act | 2 act on B | 4 row bias | 8 row sums | 16 row scale | 32 accumulate | 64 batches share  */
/* the output | 128 a group queue is open; cus: compute units (<= 0: 256).  Reads host state only: works without a device.          */
int dlwp_gemm_route_name(int entry, int M, int N, int K, int lda, int ldb, int ldc, int transA, int transB, long long nbatch,
                         const long long* strides, int dtypes, const unsigned long long* addr, int flags, int per_product, int cus,
                         char* buf, int n);

/* Strided-batched form: batch z = z1*nb2 + z2 (z1 < nb1, z2 < nb2) works on A + z1*sA1 +      */
/* z2*sA2, B + z1*sB1 + z2*sB2, C (and residual) likewise; strides in floats, 0 = shared.     */
/* res_before_act != 0 adds the residual before the activation: C = act(A.B + bias + res);    */
/* preact (optional, C's layout and strides) receives the value the activation is applied to.  */
/* act: 0 none, 1 GELU, 2 ReLU, 3 soft-shrink(act_param); bias has its own batch strides.       */
/* act 4 is the backward form C = (A.B) * GELU'(z) with the saved pre-activation z passed as    */
/* `residual` (preact must be NULL): gx = g W of a Linear layer arrives already multiplied by  */
/* the derivative of the GELU that produced its input (token-MLP backward, no gelu_bwd pass).  */
/* act 5 / 6: the same with ReLU' ([z > 0]) and soft-shrink' ([|z| > act_param]): the AFNO block */
/* MLP's activations (fourcastnet.py:100-117, F.relu and F.softshrink).                        */
/* act 7 (also in dlwp_gemm / dlwp_gemm_mixed): GELU whose `preact` output (required) receives  */
/* the DERIVATIVE GELU'(A.B + bias (+ res)) instead of the pre-activation; act 8: the backward   */
/* form C = (A.B) * f with the stored factor f passed as `residual` -- the token MLP's backward  */
/* product then multiplies by what the forward call stored and evaluates no exponential.        */
/* Without an epilogue, long-K products with few output tiles are split along K (atomics).      */
/* Used for the spherical transforms (per-order Legendre matrices) and the per-degree SFNO     */
/* spectral weights, where one launch covers every (sample, order) or degree.                  */
int dlwp_gemm_batched(const float* A, const float* B, float* C, int M, int N, int K, int lda,
                      int ldb, int ldc, int transA, int transB, int nb1, int nb2, long long sA1,
                      long long sA2, long long sB1, long long sB2, long long sC1, long long sC2,
                      const float* bias, long long sBi1, long long sBi2, int act, float act_param,
                      float* preact, const float* residual, long long sR1, long long sR2,
                      int res_before_act, int accumulate, void* stream);
/* bf16 STORAGE for the token GEMMs (BASELINE configs C3-C5 train under bf16 autocast: activations and the   */
/* weights the matrix units read are bf16 in the reference, src/dlwpbench/scripts/train.py:120-135 autocast).   */
/* dlwp_gemm / dlwp_gemm_batched with a storage mask `dtypes`: 1 = A, 2 = B, 4 = C and preact, 8 = residual   */
/* point at bf16 (2-byte) arrays; leading dimensions and batch strides stay in ELEMENTS.  Products accumulate  */
/* in fp32 and the epilogue (bias, activation, residual) runs in fp32 before the output is rounded.  A bf16    */
/* output cannot be accumulated into and is never split along K.  Unset bits are fp32 as before.               */
int dlwp_gemm_mixed(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb,
                    int ldc, int transA, int transB, const float* bias, int act, void* preact,
                    const void* residual, int accumulate, float* rowsum, int dtypes, void* stream);
int dlwp_gemm_batched_mixed(const void* A, const void* B, void* C, int M, int N, int K, int lda,
                            int ldb, int ldc, int transA, int transB, int nb1, int nb2,
                            long long sA1, long long sA2, long long sB1, long long sB2,
                            long long sC1, long long sC2, const float* bias, long long sBi1,
                            long long sBi2, int act, float act_param, void* preact,
                            const void* residual, long long sR1, long long sR2, int res_before_act,
                            int accumulate, int dtypes, void* stream);
/* Stochastic depth inside the last product of a residual branch (timm DropPath as the reference's Swin / Pangu */
/* blocks apply it: x = shortcut + drop_path(branch(x)), nsbench swin_transformer.py:255-256, dlwpbench         */
/* panguweather.py:317-323): C = (op(A) op(B) + bias) * row_scale[m / rows_per_scale] + residual, row_scale one   */
/* fp32 number per sample (0 or 1 / keep), rows_per_scale = tokens per sample.  Storage mask as dlwp_gemm_mixed.  */
/* No activation, pre-activation output, accumulation or row sums in this form.                                   */
int dlwp_gemm_rowscale(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb,
                       int ldc, int transA, int transB, const float* bias, const void* residual,
                       const float* row_scale, int rows_per_scale, int dtypes, void* stream);
/* dst[i] = bf16(src[i]) (round to nearest even): the per-step bf16 copy of the flat fp32 master weights.     */
int dlwp_cast_bf16(const float* src, void* dst, long long n, void* stream);
/* Transposed bf16 copies of a list of fp32 matrices inside two flat buffers, one launch (round 6): matrix m is src_base[descs[4m]      */
/* ...] viewed [rows = descs[4m+2]][cols = descs[4m+3]], its copy dst_base[descs[4m+1] ...] viewed [cols][rows] (bf16).  descs is a    */
/* DEVICE array of n x 4 64-bit integers; max_tiles = the largest ceil(rows/64) * ceil(cols/64).  The per-step [in][out] copies of    */
/* the Linear weights the input-gradient products read (reference: autograd's gx = g W for torch.nn.Linear, token layers of           */
/* swin_transformer.py / panguweather.py / fourcastnet.py).                                                                             */
int dlwp_transpose_cast_bf16_many(const float* src_base, void* dst_base, const long long* descs, int n, int max_tiles, void* stream);
/* dst[s][i] = bf16(src[s][i] * scale[s]), i < per_sample (a multiple of 4): the backward of dlwp_gemm_rowscale's */
/* scale on the way into the branch's bf16 products.                                                              */
int dlwp_cast_bf16_scaled(const float* src, const float* scale, void* dst, int nsamples, long long per_sample,
                          void* stream);
/* Fused real spherical harmonic transforms on channels-last fields (torch_harmonics.RealSHT /  */
/* InverseRealSHT, constructed at src/dlwpbench/models/fno/fno.py:183-200 and                   */
/* models/fourcastnet/fourcastnet.py:411-428): longitude DFT and Legendre   */
/* transform in one launch, the (latitude x order) plane stays in LDS.                          */
/*   analysis : x [B][nlat][nlon][C] -> X [lmax][B][mmax][2][C]                                 */
/*              T[k][q][c] = sum_n A1[q][n] x[b][k][n][c]   (A1 [2 mmax][nlon], q = 2m + re|im)  */
/*              X[l][b][m][ri][c] = sum_k A2[m][l][k] T[k][2m+ri][c]   (A2 [mmax][lmax][nlat])   */
/*   synthesis: X -> x, T[k][2m+ri][c] = sum_l S1[m][l][k] X[l][b][m][ri][c],                   */
/*              x[b][k][n][c] = sum_q S2[q][n] T[k][q][c]; tables given TRANSPOSED:             */
/*              S1t [mmax][nlat][lmax], S2t [nlon][2 mmax].                                     */
/* The adjoint of analysis(A1, A2) is synthesis(S1 = A2, S2 = A1) and vice versa (backward      */
/* passes).  dlwp_sht_fused_supported tells whether a shape fits (C % 16 == 0, mmax % 8 == 0,   */
/* nlon <= 128, nlat <= 64, lmax <= 64, all multiples of 4; tables 16-byte aligned); other      */
/* shapes use dlwp_gemm_batched.                                                                */
int dlwp_sht_fused_supported(int nlat, int nlon, int C, int mmax, int lmax);
int dlwp_sht_analysis(const float* x, const float* A1, const float* A2, float* X, int B, int nlat,
                      int nlon, int C, int mmax, int lmax, void* stream);
int dlwp_sht_synthesis(const float* X, const float* S1t, const float* S2t, float* x, int B, int nlat,
                       int nlon, int C, int mmax, int lmax, void* stream);
/* The same two transforms on the bf16 matrix cores for the bf16-storage chain (csrc/sht_bf16.hip): x fp32, X bf16, tables    */
/* bf16 with the contraction index contiguous: analysis A1 [2 mmax][nlon], A2 [mmax][lmax][nlat]; synthesis S1t                */
/* [mmax][nlat][lmax] (note: the TRANSPOSED Legendre table) and S2 [nlon][2 mmax] (NOT transposed); `residual` (nullable,     */
/* x's layout) is added to the synthesised field (the skip gradient in the backward pass of a forked analysis).               */
/* dlwp_sht_bf16_supported: C % 16 == 0, nlat / nlon / lmax / 2 mmax multiples of 8, nlat <= 64, nlon <= 128, lmax <= 64 and    */
/* the spectrum image within the LDS; other shapes use dlwp_gemm_batched_mixed.                                               */
int dlwp_sht_bf16_supported(int nlat, int nlon, int C, int mmax, int lmax);
int dlwp_sht_analysis_bf16(const float* x, const void* A1, const void* A2, void* X, int B, int nlat, int nlon, int C, int mmax,
                           int lmax, void* stream);
int dlwp_sht_synthesis_bf16(const void* X, const void* S1t, const void* S2, const float* residual, float* x, int B, int nlat,
                            int nlon, int C, int mmax, int lmax, void* stream);
/* The same with flags.  DLWP_SHT_TRIANGULAR: the caller guarantees X[l][.][m] = 0 for every order m > l (a spectrum that RealSHT  */
/* produced, its image under the per-degree weights of dlwp_dhconv_apply, or the gradient of either): those entries are not     */
/* read (48 % of the image at lmax = mmax = 32); with other spectra the flag gives wrong results.                               */
/* DLWP_SHT_FIELD_BF16: the FIELD tensor (the synthesis output x, which then takes no residual; the analysis input x) is a bf16  */
/* array in x's layout instead of fp32 -- for fields whose only other user is a bf16-operand kernel (the output y of an SFNO      */
/* block's spectral filter, read once by dlwp_sfno_tail_fwd; the gradient the tail's backward call leaves in gt_lp).             */
#define DLWP_SHT_TRIANGULAR 1
#define DLWP_SHT_FIELD_BF16 2
int dlwp_sht_synthesis_bf16_ex(const void* X, const void* S1t, const void* S2, const float* residual, void* x, int B, int nlat,
                               int nlon, int C, int mmax, int lmax, int flags, void* stream);
int dlwp_sht_analysis_bf16_ex(const void* x, const void* A1, const void* A2, void* X, int B, int nlat, int nlon, int C, int mmax,
                              int lmax, int flags, void* stream);
/* SFNO "driscoll-healy" spectral weights (torch_harmonics, constructed at                    */
/* src/dlwpbench/models/fno/fno.py:183-200): w [Cin][Cout][L][2] complex, one matrix per       */
/* degree l.  expand: wexp[l] = [[Wr, Wi], [-Wi, Wr]] as a real [2Cin][2Cout] matrix, so that   */
/* the complex contraction "bixy,iox->boxy" is one dlwp_gemm_batched over l on rows            */
/* [Xr | Xi]; fold: gw += the complex gradient read back from the [L][2Cin][2Cout] GEMM result. */
int dlwp_cweight_expand(const float* w, float* wexp, int Cin, int Cout, int L, void* stream);
int dlwp_cweight_fold(const float* gexp, float* gw, int Cin, int Cout, int L, void* stream);
/* The same contraction as dedicated bf16 kernels on spectra X [L][rows][C] whose rows are (sample, order, re | im) -- the        */
/* (re, im) parts of a complex row are two consecutive rows -- without the expanded image (csrc/dhconv.hip):                    */
/*   dlwp_dhconv_pack   w [Cin][Cout][L][2] fp32 -> the forward and the backward fragment-order bf16 images                      */
/*                      (dlwp_dhconv_image_elems(Cin, Cout, L) elements each)                                                   */
/*   dlwp_dhconv_apply  Y[l] = X[l] W[:, :, l] (transposed = 0, forward image, K = Cin, N = Cout) or                            */
/*                      gX[l] = gY[l] conj(W[:, :, l])^T (transposed = 1, backward image, K = Cout, N = Cin); `rows` = B * mmax * 2; */
/*                      mmax > 0: a sample's rows are its orders 0 .. mmax - 1 and orders m > l are KNOWN to be zero (spectra  */
/*                      of the SHT): those row tiles are skipped and written as zeros; mmax = 0: dense rows                     */
/*   dlwp_dhconv_wgrad  G [L][Cin][2 Cout] fp32 = sum over nseg (X, gY) pairs (the lead times of a rollout) of conj(X)^T gY     */
/*                      per degree, real parts in columns [0, Cout), imaginary parts in [Cout, 2 Cout) (overwritten)           */
/*   dlwp_dhconv_fold   gw [Cin][Cout][L][2] += G                                                                               */
/* dlwp_dhconv_supported: Cin, Cout in {128, 256}, L <= 64; other widths use dlwp_cweight_expand + dlwp_gemm_batched_mixed.       */
int dlwp_dhconv_supported(int Cin, int Cout, int L);
long long dlwp_dhconv_image_elems(int Cin, int Cout, int L);
int dlwp_dhconv_pack(const float* w, void* fwd_img, void* bwd_img, int Cin, int Cout, int L, void* stream);
/* the same for up to 16 weights of one shape (the layers of a network) in one launch; host arrays of n device pointers */
int dlwp_dhconv_pack_many(const float* const* w, void* const* fwd_img, void* const* bwd_img, int n, int Cin, int Cout, int L,
                          void* stream);
int dlwp_dhconv_apply(const void* X, const void* image, void* Y, int L, int rows, int K, int N, int mmax, int transposed,
                      void* stream);
int dlwp_dhconv_wgrad(const void* const* X, const void* const* gY, int nseg, float* G, int L, int rows, int Cin, int Cout,
                      int mmax, void* stream);
int dlwp_dhconv_fold(const float* G, float* gw, int Cin, int Cout, int L, void* stream);
/* The tail of an SFNO block as ONE launch per direction (csrc/mlp_chain.hip; the block is      */
/* torch_harmonics' SphericalFourierNeuralOperatorBlock, constructed at                         */
/* src/dlwpbench/models/fno/fno.py:183-200 and models/fourcastnet/fourcastnet.py:411-428,        */
/* SURVEY.md App. A-2): with y = the spectral filter's output and x = the block input,           */
/*     z0 = y + x Ws^T + bs,  t = GELU(z0),  z1 = t W1^T + b1,  h = GELU(z1),                     */
/*     out = h W2^T + b2 (+ x when outer)                                                       */
/* and, given g = d loss / d out,                                                               */
/*     gh = (g W2) * GELU'(z1),  gt = (gh W1) * GELU'(z0) (= d / d y),  gx = gt Ws (+ g).        */
/* Tokens are rows: x, y, out, g, gt, gx [T][C] fp32; z0, t [T][C] and z1, h, gh [T][hidden]    */
/* bf16 arrays; x_lp / g_lp (nullable) and gt_lp receive bf16 copies of x / g / gt for the       */
/* weight-gradient products.  Arithmetic: bf16 operands, fp32 accumulation and epilogues.        */
/* Round 5: the arrays the argument structs call z0 / z1 hold the DERIVATIVES GELU'(z0) and      */
/* GELU'(z1), evaluated by the forward call from the fp32 pre-activations together with the      */
/* activations; the backward call multiplies by them (no exponential / reciprocal per element    */
/* there).  They are opaque to the caller: forward output, backward input.                        */
/* The six weight matrices are read from fragment-order bf16 images built by                    */
/* dlwp_mlp_chain_pack: image of W' [rows][cols] with W' = W (transpose 0, W row-major           */
/* [rows][cols]) or W^T (transpose 1, W row-major [cols][rows]); rows % 16 == 0, cols % 32 == 0, */
/* rows * cols bf16 elements.  Forward images: Ws [C][C], W1 [hidden][C], W2 [C][hidden] as they  */
/* are; backward images: the transposes W2^T [hidden][C], W1^T [C][hidden], Ws^T [C][C].          */
/* dlwp_mlp_chain_supported: (C, hidden) pairs with a compiled kernel (256/512, 128/256,         */
/* 64/128); other widths use three dlwp_gemm_mixed calls per direction.                          */
typedef struct dlwp_sfno_tail_fwd_args {
    const float *x, *y;                     /* [T][C] */
    const void *ws_img, *w1_img, *w2_img;   /* dlwp_mlp_chain_pack images */
    const float *bs, *b1, *b2;              /* [C], [hidden], [C]; nullable */
    void *x_lp;                             /* [T][C] bf16, nullable */
    void *z0, *t, *z1, *h;                  /* bf16 outputs: GELU'(z0) [T][C], t [T][C], GELU'(z1) [T][hidden], h [T][hidden] */
    float *out;                             /* [T][C] */
    int T, C, hidden, outer;
    int y_bf16;                             /* != 0: y is a bf16 array [T][C] (dlwp_sht_synthesis_bf16_ex with DLWP_SHT_FIELD_BF16) */
} dlwp_sfno_tail_fwd_args;
typedef struct dlwp_sfno_tail_bwd_args {
    const float *g;                         /* [T][C] */
    const void *w2t_img, *w1t_img, *wst_img;
    const void *z1, *z0;                    /* the forward call's z1 / z0 arrays (activation derivatives, bf16) */
    void *g_lp;                             /* [T][C] bf16, nullable */
    void *gh;                               /* [T][hidden] bf16 */
    float *gt;                              /* [T][C]; nullable: only the bf16 copy gt_lp is written */
    void *gt_lp;                            /* [T][C] bf16 */
    float *gx;                              /* [T][C] */
    int T, C, hidden, outer;
} dlwp_sfno_tail_bwd_args;
int dlwp_mlp_chain_supported(int C, int hidden);
int dlwp_mlp_chain_pack(const float* W, int rows, int cols, int transpose, void* image, void* stream);
/* all six images of a tail in one launch: images [6][C * hidden] bf16 = forward Ws, W1, W2, backward W2^T, W1^T, Ws^T  */
/* (the two C x C images use the front of their slots); ws [C][C], w1 [hidden][C], w2 [C][hidden] fp32.               */
int dlwp_sfno_tail_pack(const float* ws, const float* w1, const float* w2, int C, int hidden, void* images, void* stream);
/* the same for up to 8 block tails of equal widths in ONE launch (images[b]: the 6-image slot of block b) */
int dlwp_sfno_tail_pack_many(const float* const* ws, const float* const* w1, const float* const* w2, int n, int C, int hidden,
                             void* const* images, void* stream);
int dlwp_sfno_tail_fwd(const dlwp_sfno_tail_fwd_args* args, void* stream);
int dlwp_sfno_tail_bwd(const dlwp_sfno_tail_bwd_args* args, void* stream);
/* Token MLP y = fc2(GELU(fc1 x)) (+ residual) of the AFNO / Swin / Pangu blocks (nsbench/models/fourcastnet/fourcastnet.py:40-56, */
/* swintransformer/swin_transformer.py:25-48) and its input-gradient chain as ONE launch per direction for wide hidden layers      */
/* (csrc/mlp_stream.hip): a workgroup owns 64 tokens and walks the hidden layer in chunks of 128 with the output accumulators in    */
/* registers; z, h ([T][hidden] bf16) are written for the other pass and the weight gradients but never read back as operands.     */
/*   pack: images [4][E * hidden] bf16 = forward W1 [hidden][E], W2 [E][hidden], backward W2^T, W1^T (dlwp_mlp_chain_pack order)   */
/*   fwd : x [T][E] (bf16 array when x_bf16, else fp32 with an optional bf16 copy x_lp) -> z, h, y [T][E] fp32 (+ residual)        */
/*   bwd : g [T][E] fp32 (-> bf16 copy g_lp, nullable), z -> gh [T][hidden] bf16, gx [T][E] (bf16 array when gx_bf16)              */
/* dlwp_mlp_stream_supported: E = 768, hidden a multiple of 128; other widths use two dlwp_gemm_mixed calls per direction.          */
int dlwp_mlp_stream_supported(int E, int hidden);
int dlwp_mlp_stream_pack(const float* w1, const float* w2, int E, int hidden, void* images, void* stream);
int dlwp_mlp_stream_fwd(const void* x, int x_bf16, void* x_lp, const void* w1_img, const float* b1, const void* w2_img, const float* b2,
                        const float* residual, void* z, void* h, float* y, int T, int E, int hidden, void* stream);
int dlwp_mlp_stream_bwd(const float* g, void* g_lp, const void* w2t_img, const void* w1t_img, const void* z, void* gh, void* gx,
                        int gx_bf16, int T, int E, int hidden, void* stream);
/* SFNO encoder / decoder with the rollout's frame assembly, ONE launch per direction each (csrc/sfno_io.hip).  Reference:   */
/* SphericalFourierNeuralOperatorNet's encoder / decoder 1x1-convolution MLPs, position embedding and big skip (constructed at */
/* src/dlwpbench/models/fno/fno.py:183-200) inside SFNO2DModule.forward's loop (fno.py:217-259; clean form unet.py:64-111):    */
/*   x_t = cat(constants[:, 0], prescribed[:, t-1], frame);  t0 = W2e GELU(W1e x_t + b1e) + pos;                               */
/*   y = W2d GELU(Wd [t ; x_t] + bd);  out = frame + y.                                                                        */
/* Token tensors are rows (tokens [T][E] fp32, T = B * HW); frames and gradients of frames are NCHW planes given by the        */
/* pointer of sample 0 and a batch stride in floats; tok_lp [T][DLWP_SFNO_IO_KP] holds the gathered input channels of a token  */
/* as bf16 (zero beyond the real channels).  z, h ([T][E] bf16): the hidden layer's pre-activation and activation (forward:   */
/* written; backward: z read, h receives the hidden gradient gh).  One argument struct serves the four calls:                 */
/*   encode_fwd  src* (up to three plane groups) -> tok_lp, z, h, tokens = t0 (+ pos [HW][E], nullable)                        */
/*   encode_bwd  tokens = g (d loss / d t0) -> tokens_lp (bf16 copy of g), h = gh; the token gradient gh W1e (+ tok_grad, the   */
/*               decoder's share, nullable) has its channels frame_c0 .. frame_c0 + frame_c - 1 written to `frame`             */
/*               (+ frame_add, nullable: the gradient that reached the same frame through the decoder's residual)             */
/*   decode_fwd  tokens = t, tok_lp -> tokens_lp (bf16 copy of t), z, h, frame[b][c] = frame_add[b][c] + y (c < frame_c)       */
/*   decode_bwd  src[0] = g_out (src_c[0] planes) -> tok_lp (bf16 rows of g_out), h = gh, tokens = g_t, tok_grad = g_tok        */
/* Weight images: dlwp_sfno_io_pack builds the eight zero-padded fragment-order images (slot i at images + i *                */
/* dlwp_sfno_io_image_elems(E) bf16 elements: encode fwd 1 / 2, encode bwd 1 / 2, decode fwd 1 / 2, decode bwd 1 / 2) from     */
/* enc_w1 [E][in], enc_w2 [E][E], dec_w1 [E][E (+ in with big_skip)], dec_w2 [out][E].  bf16 operands, fp32 accumulation.     */
#define DLWP_SFNO_IO_KP 32
typedef struct dlwp_sfno_io_args {
    const float* src[3];
    long long src_bs[3];
    int src_c[3];
    int HW, T, E;
    float* tokens;
    void* tokens_lp;
    void* tok_lp;
    const void *w1_img, *w2_img;
    const float *bias, *pos;
    void *z, *h;
    float* frame;
    long long frame_bs;
    int frame_c, frame_c0;
    const float* frame_add;
    long long frame_add_bs;
    float* tok_grad;
} dlwp_sfno_io_args;
int dlwp_sfno_io_supported(int E, int in_chans, int out_chans);
long long dlwp_sfno_io_image_elems(int E);
int dlwp_sfno_io_pack(const float* enc_w1, const float* enc_w2, const float* dec_w1, const float* dec_w2, int E, int in_chans,
                      int out_chans, int big_skip, void* images, void* stream);
int dlwp_sfno_encode_fwd(const dlwp_sfno_io_args* args, void* stream);
int dlwp_sfno_encode_bwd(const dlwp_sfno_io_args* args, void* stream);
int dlwp_sfno_decode_fwd(const dlwp_sfno_io_args* args, void* stream);
int dlwp_sfno_decode_bwd(const dlwp_sfno_io_args* args, void* stream);
/* LayerNorm over the last dimension of x [T,C]; mean/rstd [T] are saved for backward.       */
int dlwp_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y,
                       float* mean, float* rstd, int T, int C, float eps, void* stream);
/* The same with the output stored as bf16 (y_bf16 != 0: y is a 2-byte array) for LayerNorms whose only   */
/* reader is a GEMM under bf16 storage (dlwp_gemm_mixed); statistics and the backward pass stay fp32.       */
int dlwp_layernorm_fwd_ex(const float* x, const float* gamma, const float* beta, void* y, float* mean,
                          float* rstd, int T, int C, float eps, int y_bf16, void* stream);
/* Backward of a LayerNorm whose bf16 output fed a GEMM: the upstream gradient arrives as a bf16 array      */
/* (gy_bf16 != 0) straight from that GEMM's input-gradient product; gadd as in dlwp_layernorm_bwd_res.      */
int dlwp_layernorm_bwd_ex(const float* x, const float* gamma, const float* mean, const float* rstd,
                          const void* gy, int gy_bf16, const float* gadd, float* gx, float* ggamma,
                          float* gbeta, int T, int C, void* stream);

/* As dlwp_layernorm_bwd_ex, with a second output (round 6): gx_bf16[t][c] = bf16(gx[t][c] * row_scale[t / rows_per_sample]) -- the      */
/* gradient the residual branch that ENDS in this stream wants for its backward products (per-sample stochastic-depth scale, bf16       */
/* operands; reference: DropPath in Block.forward, swin_transformer.py:255-256, whose backward scales the branch gradient), written    */
/* from the registers that hold gx instead of by a separate pass over it.  row_scale NULL: a plain bf16 copy.                           */
int dlwp_layernorm_bwd_lowp(const float* x, const float* gamma, const float* mean, const float* rstd, const void* gy, int gy_bf16,
                            const float* gadd, float* gx, float* ggamma, float* gbeta, int T, int C, void* gx_bf16,
                            const float* row_scale, int rows_per_sample, void* stream);
/* gx written; ggamma/gbeta ACCUMULATED into.  C <= 2048.                                    */
int dlwp_layernorm_bwd(const float* x, const float* gamma, const float* mean, const float* rstd,
                       const float* gy, float* gx, float* ggamma, float* gbeta, int T, int C,
                       void* stream);
/* The same with gx = (LayerNorm backward) + gadd [T,C] (nullable): in the pre-norm residual   */
/* blocks (`x + f(norm(x))`: nsbench fourcastnet.py:156-165, swin_transformer.py:229-256;       */
/* dlwpbench panguweather.py:143-159) the gradient of the block input is the sum of the residual */
/* branch's and the norm's -- formed here instead of by a separate elementwise add.              */
int dlwp_layernorm_bwd_res(const float* x, const float* gamma, const float* mean, const float* rstd,
                           const float* gy, const float* gadd, float* gx, float* ggamma,
                           float* gbeta, int T, int C, void* stream);
/* Instance normalisation of channels-last tokens x [B][P][C]: per (sample, channel) mean / biased       */
/* variance over the P = H*W tokens, y = (x - mean) rstd gamma + beta (+ residual, same layout, optional).  */
/* Replaces nn.InstanceNorm2d(embed_dim, eps, affine=True) inside torch_harmonics' SFNO                      */
/* (normalization_layer="instance_norm": src/dlwpbench/configs/model/fourcastnetv2.yaml:23, constructed at   */
/* src/dlwpbench/models/fourcastnet/fourcastnet.py:411-428).  stats [B][C][2] receives (mean, rstd).         */
int dlwp_instnorm_fwd(const float* x, const float* gamma, const float* beta, const float* residual,
                      float* y, float* stats, int B, int P, int C, float eps, void* stream);
/* gx written; ggamma / gbeta ACCUMULATED into; work: scratch [B][C][2].                                    */
int dlwp_instnorm_bwd(const float* x, const float* gamma, const float* stats, const float* gy, float* gx,
                      float* ggamma, float* gbeta, float* work, int B, int P, int C, void* stream);
/* gz = gy * gelu'(z) (exact erf GELU)                                                       */
int dlwp_gelu_bwd(const float* z, const float* gy, float* gz, long long n, void* stream);
/* gz = gy * act'(z) for the epilogue activations of dlwp_gemm_batched (1 GELU, 2 ReLU, 3 soft-shrink) */
int dlwp_act_bwd(const float* z, const float* gy, float* gz, long long n, int act, float act_param,
                 void* stream);
/* Stochastic depth (timm DropPath: src/nsbench/models/swintransformer/swin_transformer.py:193,   */
/* 255-256; dlwpbench twin :192,261-262; panguweather.py:262-323): the per-sample keep mask, already    */
/* divided by the keep probability, scales a residual branch: out[b][i] = x[b][i] + scale[b] t[b][i]    */
/* (x may be NULL: plain scaling, which is also the backward of the branch: gt = scale[b] g).           */
/* t, x, out: [B][n]; scale: [B] device floats, or NULL for unit scales (a plain fused add).              */
int dlwp_scale_rows_add(const float* t, const float* scale, const float* x, float* out, int B,
                        long long n, void* stream);
/* out[b][i] = t[b][i] + p[i]: a learned position embedding [n] added to every sample's tokens   */
/* (`x = patch_embed(x) + pos_embed`, src/nsbench/models/fourcastnet/fourcastnet.py:253; dlwpbench */
/* twin).  Its parameter gradient is dlwp_colsum over the batch.                                   */
int dlwp_add_bcast(const float* t, const float* p, float* out, int B, long long n, void* stream);
/* out[n] += sum_t g[t][n]   (bias gradients)                                                */
int dlwp_colsum(const float* g, float* out, int T, int N, void* stream);
/* dst[r][c] += src[r * src_rs + c * src_cs] (dst row pitch dst_ld) for up to DLWP_ADD2D_MAX small matrices in ONE launch: */
/* padded, concatenated or transposed temporary gradients handed to the parameters' gradient buffers (the encoder's  */
/* / decoder's 1x1 convolution weights and the position embedding of SFNO2DModule, dlwpbench fno.py:217-259).        */
#define DLWP_ADD2D_MAX 8
typedef struct dlwp_add2d_desc {
    float* dst;
    const float* src;
    long long dst_ld, src_rs, src_cs;
    int rows, cols;
} dlwp_add2d_desc;
int dlwp_add2d_many(const dlwp_add2d_desc* descs, int n, void* stream);
/* out[n] += sum_t g[t][n] for a bf16 array g (tall form, T > 16)                                                      */
int dlwp_colsum_bf16(const void* g, float* out, int T, int N, void* stream);
/* the same with overwrite != 0: out[n] = sum_t g[t][n] (the first of several accumulating calls needs no zero fill) */
int dlwp_colsum_ex(const float* g, float* out, int T, int N, int overwrite, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Complex mode-n product for Tucker-factorised spectral weights (TFNO, dlwpbench/models/   */
/* fno/fno.py:136-146): out[O,N,I] = sum_r in[O,r,I] * U[N,r]; complex = interleaved re/im. */
/* The factorised weight core x1 U_i x2 U_o x3 U_x x4 U_y is expanded into the dense layout   */
/* of dlwp_fno_block_* once per optimizer step.  _bwd writes gin and gU.                      */
int dlwp_cmode_product(const float* in, const float* U, float* out, int O, int R, int N, int I,
                       void* stream);
int dlwp_cmode_product_bwd(const float* in, const float* U, const float* gout, float* gin,
                           float* gU, int O, int R, int N, int I, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Data-parallel exchange over RCCL (xGMI).  The reference trains single-process            */
/* (nsbench/scripts/train.py:36,66); sharding trajectory samples over the GPUs of a node is a  */
/* build addition whose only collective is ONE sum all-reduce of the flat fp32  */
/* gradient buffer per optimizer step (then Adam with grad_scale = 1 / world).  One communicator */
/* per process / GPU: rank 0 calls dlwp_comm_unique_id and hands the 128 bytes to every rank     */
/* (any side channel), every rank calls dlwp_comm_create (blocks until all have joined).         */
/* Collectives are enqueued on the caller's stream.  librccl is loaded at the first call.        */
typedef struct dlwp_comm dlwp_comm;
int dlwp_comm_unique_id(void* out128);
int dlwp_comm_create(const void* unique_id128, int rank, int world, dlwp_comm** out);
void dlwp_comm_destroy(dlwp_comm* comm);
/* buf[0:n] <- sum over ranks (in place)                                                   */
int dlwp_comm_allreduce(dlwp_comm* comm, float* buf, long long n, void* stream);
/* buf[0:n] <- root's buf (initial parameters, Adam state on resume)                       */
int dlwp_comm_broadcast(dlwp_comm* comm, float* buf, long long n, int root, void* stream);

/* ------------------------------------------------------------------------------------ */
/* 3 x 3 convolutions (stride 1, same size) and the ConvLSTM cell (csrc/conv3x3.hip).  Replace every       */
/* nn.Conv2d(kernel_size=3, padding=1, padding_mode="circular") of src/nsbench/models/convlstm/convlstm.py */
/* (:31-39, :105-128) and the CylinderPad + nn.Conv2d pairs of src/dlwpbench/models/convlstm/convlstm.py.   */
/* Activations are channels-last fp32 [B][H][W][C]; fp32 operands on the exact-fp32 MFMA, fp32 sums.        */
/* Codes: padding per axis 0 = zeros, 1 = circular, 2 = HEALPix (both axes at once, see below);            */
/* activation 0 = none, 1 = tanh, 2 = relu;                                                                */
/* image kind 0 = forward, 1 = forward of a cell weight (gate columns interleaved), 2 = input gradient.    */
/* No padded tensor and no cat(x, h_prev) is ever written: the halo is resolved while a tile is staged.    */
/*                                                                                                         */
/* Floats of the packed image of a weight [Cout][Cin][3][3] (negative: bad argument).                      */
long long dlwp_conv3x3_image_floats(int Cin, int Cout, int kind);
/* img <- the image of w [Cout][Cin][3][3] (nn.Conv2d's layout, which stays the parameter); written whole. */
int dlwp_conv3x3_pack(const float* w, float* img, int Cin, int Cout, int kind, void* stream);
/* y = act(conv3x3(cat(x1 [..][C1], x2 [..][C2]), w) + bias): output columns [0, N1) are WRITTEN to        */
/* y1 [..][N1], columns [N1, N1 + N2) to y2 [..][N2]; x2 (with C2 = 0), bias, and one of y1 / y2 may be    */
/* NULL (that destination is skipped).  wimg: kind 0 image of [N1 + N2][C1 + C2][3][3].  With the kind 2    */
/* image of a weight [C1][N1 + N2][3][3] the same call is the INPUT GRADIENT of that convolution: x1 = dz,   */
/* y1 = gradient of its first input, y2 = gradient of its second (the cell: dx and dh_prev).                */
int dlwp_conv3x3_fwd(const float* x1, const float* x2, const float* wimg, const float* bias, float* y1,
                     float* y2, int B, int H, int W, int C1, int C2, int N1, int N2, int pad_h, int pad_w,
                     int act, void* stream);
/* One ConvLSTM cell step (convlstm.py:67-80): z = conv3x3(cat(x [..][Cx], h_prev [..][hid])) + bias with   */
/* output channels (input, i, f, o) in blocks of hid; c = sig(f) c_prev + sig(i) tanh(input),                */
/* h = sig(o) tanh(c).  wimg: kind 1 image of [4 hid][Cx + hid][3][3].  WRITES h, c [..][hid] and (unless    */
/* NULL) the activated gates [..][4 hid] for the backward pass; the pre-activations never reach memory.      */
/* h_prev / c_prev NULL = zero state (the recurrent half of the product is skipped).                         */
int dlwp_convlstm_cell_fwd(const float* x, const float* h_prev, const float* wimg, const float* bias,
                           const float* c_prev, float* h, float* c, float* gates, int B, int H, int W, int Cx,
                           int hid, int pad_h, int pad_w, void* stream);
/* Gate backward of the cell, element-wise: from dh, dc (either may be NULL = zero), the stored gates,      */
/* c_prev (NULL = zero) and c it WRITES dz [npix][4 hid] (pre-activation gradient, the weight's channel       */
/* order) and dc_prev [npix][hid].                                                                          */
int dlwp_convlstm_gate_bwd(const float* dh, const float* dc, const float* gates, const float* c_prev,
                           const float* c, float* dz, float* dc_prev, long long npix, int hid, void* stream);
/* dz = gy * act'(y) from the activation's OUTPUT y (1: 1 - y^2, 2: y > 0); written.                       */
int dlwp_conv3x3_act_bwd(const float* y, const float* gy, float* dz, long long n, int act, void* stream);
/* Weight and bias gradient: gw [Cout][C1 + C2][3][3] += sum_pixels in[p + tap][ci] dz[p][co] with the       */
/* forward's halo rules, gb [Cout] += sum_pixels dz (NULL: none).  Both are ACCUMULATED into.  ws: scratch    */
/* of dlwp_conv3x3_wgrad_ws_floats floats (per-workgroup partial sums, folded in a fixed order: no atomics,   */
/* repeated launches are bit-identical).                                                                    */
long long dlwp_conv3x3_wgrad_ws_floats(int B, int H, int W, int Cin, int Cout);
int dlwp_conv3x3_wgrad(const float* x1, const float* x2, const float* dz, float* ws, float* gw, float* gb, int B,
                       int H, int W, int C1, int C2, int Cout, int pad_h, int pad_w, void* stream);
/* HEALPix padding (code 2 on BOTH axes; HEALPixPadding(1) of src/dlwpbench/utils/healpix.py in front of    */
/* every nn.Conv2d(3) of a HEALPixLayer): B = 12 * spheres square faces [B][n][n][C], face index fastest.  */
/* Every cell of the one-pixel ring around a face is one pixel of a neighbour face (some faces are seen     */
/* rotated) or, for the top-left / bottom-right corner cell of the four equatorial faces, the mean of two;  */
/* dlwp_conv3x3_fwd, dlwp_convlstm_cell_fwd and dlwp_conv3x3_wgrad resolve it while they stage a tile.       */
/* They refuse (DLWP_E_INVALID) the code on one axis only, B % 12 != 0, H != W and H < 2.                   */
/*                                                                                                         */
/* HOST function, no GPU: out [12][4 n + 4][2] <- the source pixels ((face * n + y) * n + x within the       */
/* sphere; second entry -1 unless the cell is a mean of two) of every ring cell, from the closed form the    */
/* kernels run.  Ring cell order of the padded (n + 2) x (n + 2) face: top row, bottom row, then the left    */
/* and the right column without their corners.                                                             */
int dlwp_hpx_halo_sources(int n, int* out);
/* Input gradient under HEALPix padding: dx = P^T (full transposed convolution of dz), which is NOT the      */
/* convolution with the flipped weight and the same padding.  Two launches: the kind 2 image product over    */
/* the padded domain of every face into ws [B][n + 2][n + 2][C1 + C2] (dlwp_conv3x3_hpx_dgrad_ws_floats),     */
/* then a gather that WRITES g1 [B][n][n][C1] and g2 [..][C2] (either may be NULL): every pixel takes its     */
/* interior value plus, in the table's order, the ring cells that read it -- no atomics, repeated launches   */
/* are bit-identical.  table: device int [12][4 n - 4][4], per border pixel of a face (top row, bottom row,  */
/* left, right column without corners) up to four entries (cell << 1) | half with                           */
/* cell = (face * (n + 2) + pr) * (n + 2) + pc within the sphere and half = 1 for weight 0.5; -1 = none.      */
long long dlwp_conv3x3_hpx_dgrad_ws_floats(int B, int n, int Cin);
int dlwp_conv3x3_hpx_dgrad(const float* dz, const float* wimg, const int* table, float* ws, float* g1, float* g2,
                           int B, int n, int Cout, int C1, int C2, void* stream);
/* Face-packed HEALPix 3 x 3 kernels for small faces (csrc/conv3x3_hpx_packed.hip), n in {1, 2, 4, 8}: the M  */
/* axis of a workgroup is the pixels of several whole consecutive faces of [B][n][n][C] (64 faces at n = 1,  */
/* 32 at 2, 8 at 4, 2 at 8) instead of one 8 x 16 tile of one face.  Same packed weight images (kinds 0 and  */
/* 2), same arithmetic.  Other n <= 8 and n > 8: DLWP_E_UNSUPPORTED; B % 12 != 0 or H != W: DLWP_E_INVALID.   */
/* fwd: dlwp_conv3x3_fwd's arguments without the padding codes.                                              */
int dlwp_conv3x3_hpxp_fwd(const float* x1, const float* x2, const float* wimg, const float* bias, float* y1, float* y2,
                          int B, int H, int W, int C1, int C2, int N1, int N2, int act, void* stream);
/* dgrad: as dlwp_conv3x3_hpx_dgrad (product over the padded domain into ws, then the gather fold), but the  */
/* table is conv_ops.hpx_fold_rows(n): device int [12][n * n][R], per pixel of a face (row-major) the ring    */
/* cells that read it in ascending order, (cell << 1) | half as above, -1 = none; R = 10 at n = 1, else 4.    */
long long dlwp_conv3x3_hpxp_dgrad_ws_floats(int B, int n, int Cin);
int dlwp_conv3x3_hpxp_dgrad(const float* dz, const float* wimg, const int* table, int R, float* ws, float* g1, float* g2,
                            int B, int n, int Cout, int C1, int C2, void* stream);
/* wgrad: as dlwp_conv3x3_wgrad with the packed tile walk as the K axis; ws [S][9][Cin_pad][Cout_pad].        */
long long dlwp_conv3x3_hpxp_wgrad_ws_floats(int B, int n, int Cin, int Cout);
int dlwp_conv3x3_hpxp_wgrad(const float* x1, const float* x2, const float* dz, float* ws, float* gw, float* gb, int B,
                            int n, int C1, int C2, int Cout, void* stream);

/* ------------------------------------------------------------------------------------ */
/* The U-Net layers that are not 3 x 3 convolutions (csrc/unet_ops.hip): AvgPool2d(2, 2), ConvTranspose2d(2, 2)  */
/* and the 1 x 1 output convolution of src/{nsbench,dlwpbench}/models/unet/unet.py.  Channels-last fp32           */
/* [B][H][W][C] like the 3 x 3 kernels; the products run on the exact-fp32 MFMA.  No atomics anywhere: repeated   */
/* launches on the same operands are bit-identical.                                                              */
/*                                                                                                               */
/* y [B][H/2][W/2][C] = 0.25 * (((a + b) + c) + d) over the 2 x 2 block (row-major order); H, W: the UNPOOLED     */
/* size, both even (DLWP_E_UNSUPPORTED otherwise).  bwd WRITES dx [B][H][W][C] = 0.25 * dy at all four positions. */
int dlwp_avgpool2x2_fwd(const float* x, float* y, int B, int H, int W, int C, void* stream);
int dlwp_avgpool2x2_bwd(const float* dy, float* dx, int B, int H, int W, int C, void* stream);
/* y [npix][Cout] = x [npix][Cin] . w^T + bias (nn.Conv2d's [Cout][Cin][1][1]; bias nullable); dgrad WRITES        */
/* dx [npix][Cin] = dy [npix][Cout] . w.                                                                          */
int dlwp_conv1x1_fwd(const float* x, const float* w, const float* bias, float* y, long long npix, int Cin, int Cout,
                     void* stream);
int dlwp_conv1x1_dgrad(const float* dy, const float* w, float* dx, long long npix, int Cin, int Cout, void* stream);
/* ConvTranspose2d(Cin, Cout, kernel_size=2, stride=2): y [B][2H][2W][Cout], y[2i+di][2j+dj][co] =                 */
/* sum_ci x[i][j][ci] w[ci][co][di][dj] + bias[co] with w the layer's own [Cin][Cout][2][2]; H, W: the INPUT size.  */
/* dgrad WRITES dx [B][H][W][Cin] from dy [B][2H][2W][Cout].                                                       */
int dlwp_upconv2x2_fwd(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin,
                       int Cout, void* stream);
int dlwp_upconv2x2_dgrad(const float* dy, const float* w, float* dx, int B, int H, int W, int Cin, int Cout,
                         void* stream);
/* Weight and bias gradients of the two layers, ACCUMULATED into gw (the parameter's own layout) and gb [Cout]    */
/* (NULL: none; for the up-convolution the sum of dy over all four positions).  ws: scratch of *_ws_floats floats  */
/* (per-workgroup partial sums, folded in a fixed order).                                                         */
long long dlwp_conv1x1_wgrad_ws_floats(long long npix, int Cin, int Cout);
int dlwp_conv1x1_wgrad(const float* x, const float* dy, float* ws, float* gw, float* gb, long long npix, int Cin,
                       int Cout, void* stream);
long long dlwp_upconv2x2_wgrad_ws_floats(int B, int H, int W, int Cin, int Cout);
int dlwp_upconv2x2_wgrad(const float* x, const float* dy, float* ws, float* gw, float* gb, int B, int H, int W,
                         int Cin, int Cout, void* stream);

/* ---- graph kernels of the MeshGraphNet baselines (csrc/graph_ops.hip) ------------------------------------------ */
/* Reference: MeshGraphMLP / MeshEdgeBlock / MeshNodeBlock of src/{nsbench,dlwpbench}/models/graphcast/gnn_layers/    */
/* (mesh_graph_mlp.py:171-194, mesh_edge_block.py:86-94, mesh_node_block.py:83-93; concat_efeat_dgl and              */
/* agg_concat_dgl in utils.py:115-150, 340-380).  Activations are fp32 row-major [rows][width]; src, dst, the CSR    */
/* offsets and edge ids are int32 DEVICE arrays of ONE sample's graph (N nodes, E edges) whose indices the caller    */
/* has checked; sample b's node i is row b N + i, its edge k row b E + k.  No atomics: every launch is bit-          */
/* reproducible.  Every width is 1..DLWP_GRAPH_MAX_WIDTH, 1..DLWP_GRAPH_MAX_HIDDEN_LAYERS hidden layers.             */
#define DLWP_GRAPH_MAX_WIDTH 128
#define DLWP_GRAPH_MAX_HIDDEN_LAYERS 3
enum { DLWP_GRAPH_ROWS = 0, DLWP_GRAPH_EDGE = 1, DLWP_GRAPH_NODE = 2 };
enum { DLWP_GRAPH_ACT_RELU = 0, DLWP_GRAPH_ACT_SILU = 1 };
/* One launch: hidden_layers x (Linear + bias + activation), Linear + bias [, LayerNorm (biased variance, affine)    */
/* when gamma != NULL] [, + residual] on the operand rows                                                           */
/*   rows  A[r] = x[r]                                   (x [rows][De])                                              */
/*   edge  A[r] = x[r] | v[b N + src[k]] | v[b N + dst[k]]   (x = e [B E][De], v [B N][Dv]; residual: + e[r])          */
/*   node  A[r] = agg[r] | v[r],  agg[r] = sum (mean != 0: mean) of x[b E + in_eid[j]], in_ptr[i] <= j < in_ptr[i+1]   */
/*         (x = e [B E][De]; a node without in-edges gets zeros; residual: + v[r])                                   */
/* which are assembled while they are staged: the concatenation is never written.  w[l] [out_l][in_l] and b[l] are   */
/* nn.Linear's own arrays (b[l] nullable); every hidden layer has `hidden` columns.  Stored for a backward pass,     */
/* each unless NULL: hid[l] [rows][hidden] post-activation rows, xhat [rows][out] normalised rows, rstd [rows]       */
/* 1 / sigma, agg [B N][De] (node mode).                                                                             */
/* act (the LAST fields, so that a zero-initialised struct of the earlier layout means what it meant): ReLU (0), or  */
/* SiLU v s with s = 1 / (1 + exp(-v)) (MeshGraphMLP's activation_fn in GraphCastNetNS, graph_cast_net_ns.py:208-246). */
/* SiLU's derivative cannot be taken from the stored v s, so der[l] [rows][hidden] (each unless NULL, SiLU only)     */
/* receives d = s (1 + v (1 - s)); both stay finite for any finite v (-0 / 0 and v / 1 far out).                     */
typedef struct dlwp_graph_mlp_args {
    int mode, B, N, E;
    long long rows;                     /* rows mode only; edge: B E, node: B N */
    const float *x, *v;
    const int *src, *dst, *in_ptr, *in_eid;
    int De, Dv, hidden, out, hidden_layers, residual, mean;
    float eps;
    const float* w[DLWP_GRAPH_MAX_HIDDEN_LAYERS + 1];
    const float* b[DLWP_GRAPH_MAX_HIDDEN_LAYERS + 1];
    const float *gamma, *beta;
    float* y;
    float* hid[DLWP_GRAPH_MAX_HIDDEN_LAYERS];
    float *xhat, *rstd, *agg;
    int act;
    float* der[DLWP_GRAPH_MAX_HIDDEN_LAYERS];
} dlwp_graph_mlp_args;
int dlwp_graph_mlp_fwd(const dlwp_graph_mlp_args* args, void* stream);
/* LayerNorm backward from the stored rows: WRITES dz [rows][C]; ggamma / gbeta (each nullable) are ACCUMULATED      */
/* into from per-workgroup column sums folded in workgroup order.  ws: dlwp_graph_ln_bwd_ws_floats floats.           */
long long dlwp_graph_ln_bwd_ws_floats(long long rows, int C);
int dlwp_graph_ln_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dz, float* ws,
                      float* ggamma, float* gbeta, long long rows, int C, void* stream);
/* Weight and bias gradient of the FIRST Linear: gw [hidden][K0] += dz^T . A, gb [hidden] += column sums of dz      */
/* (NULL: none), with A gathered as in the forward (K0 = De | De + 2 Dv | De + Dv; node mode: x = the stored agg).  */
/* ws: dlwp_graph_wgrad0_ws_floats(rows, K0, hidden) floats of per-workgroup partial sums, folded in a fixed order.  */
long long dlwp_graph_wgrad0_ws_floats(long long rows, int K0, int hidden);
int dlwp_graph_wgrad0(int mode, const float* x, const float* v, const int* src, const int* dst, const float* dz, float* ws,
                      float* gw, float* gb, int B, int N, int E, long long rows, int De, int Dv, int hidden, void* stream);
/* Input gradient of the first Linear, dA = dz . w (w [hidden][K0]), WRITTEN in parts (each nullable):               */
/*   rows  out0 = dx [rows][De]                                                                                      */
/*   edge  out0 = de [B E][De] (+ res), out1 = per-edge d_src [B E][Dv], out2 = per-edge d_dst [B E][Dv]              */
/*   node  out0 = d_agg [B N][De], out1 = dv [B N][Dv] (+ res)                                                        */
/* res (nullable): the gradient arriving along the block's residual, in the layout of the part it is added to.       */
int dlwp_graph_dgrad0(int mode, const float* dz, const float* w, const float* res, float* out0, float* out1, float* out2,
                      int B, int N, int E, long long rows, int De, int Dv, int hidden, void* stream);
/* Input gradient of a LATER Linear with the activation's derivative applied as it is stored:                        */
/* out [rows][in] = (dz [rows][out_width] . w [out_width][in]) * mul [rows][in]   (mul NULL: dz . w alone).           */
/* One launch for dlwp_conv1x1_dgrad followed by an element-wise pass; SiLU's backward takes it with mul = der[l-1]. */
int dlwp_graph_dgrad_mul(const float* dz, const float* w, const float* mul, float* out, long long rows, int in, int out_width,
                         void* stream);
/* out[b N + i] = [add[b N + i]] + sum_j in1[b E + eid1[j]] (ptr1[i] <= j < ptr1[i+1]; mean1 != 0: divided by the     */
/* count) [+ sum_j in2[b E + eid2[j]] over the second list], rows of width C, summed in list order.  The forward     */
/* aggregation on its own (in-edges), and dv of an edge block (out-edges of d_src, in-edges of d_dst).               */
int dlwp_graph_gather_sum(const float* in1, const int* ptr1, const int* eid1, int mean1, const float* in2, const int* ptr2,
                          const int* eid2, const float* add, float* out, int B, int N, int E, int C, void* stream);
/* out[b E + k] = [add[b E + k]] + in[b N + dst[k]] (in_ptr != NULL: divided by the in-degree of dst[k]): de of a     */
/* node block from d_agg.                                                                                            */
int dlwp_graph_edge_gather(const float* in, const int* dst, const int* in_ptr, const float* add, float* out, int B, int N,
                           int E, int C, void* stream);

/* ---- wide, bipartite graph kernels of the dlwpbench GraphCastNet (csrc/graph_wide.hip) ---------------------------- */
/* The row MLPs above at widths 1..DLWP_GRAPH_WIDE_MAX_WIDTH, one Linear per launch on a (64 rows x 64 | 128 columns) */
/* grid, on graphs whose source and destination nodes are different sets (Ns, Nd nodes; the mesh graph: Ns == Nd and   */
/* vs == vd).  Reference: MeshGraphMLP / MeshGraphEdgeMLPConcat (mesh_graph_mlp.py), concat_efeat and                 */
/* aggregate_and_concat (utils.py) of src/dlwpbench/models/graphcast/gnn_layers/.  Layout, index arrays and            */
/* reproducibility as above: fp32 rows, int32 arrays of ONE sample's graph, no atomics.  Nothing above changes:        */
/* DLWP_GRAPH_MAX_WIDTH stays 128.                                                                                    */
#define DLWP_GRAPH_WIDE_MAX_WIDTH 512
#define DLWP_GRAPH_WIDE_ACT_NONE (-1)
/* The operand rows of a first Linear, assembled while they are staged (the concatenation is never written):         */
/*   rows  A[r] = x[r]                                         (x [rows][D0])                                         */
/*   edge  A[r] = x[r] | vs[b Ns + src[k]] | vd[b Nd + dst[k]]   (x = e [B E][D0], vs [B Ns][D1], vd [B Nd][D2])        */
/*   node  A[r] = x[r] | vs[r]                                 (x = agg [B Nd][D0] from dlwp_graph_wide_gather_sum,   */
/*                                                              vs = v [B Nd][D1])                                    */
/* Every part is 1..512 wide, so the fan-in K = D0 [+ D1 [+ D2]] is at most 1536.  Entry points that read shapes only */
/* (dlwp_graph_wide_dgrad, *_ws_floats) ignore the pointers.                                                          */
typedef struct dlwp_graph_wide_operand {
    int mode, B, Ns, Nd, E;
    long long rows;                     /* rows mode only; edge: B E, node: B Nd */
    const float *x, *vs, *vd;
    const int *src, *dst;
    int D0, D1, D2;
} dlwp_graph_wide_operand;
/* y [rows][N] = act(A . w^T + b) [+ res]: w [N][K] and b [N] (nullable) are nn.Linear's own arrays; act             */
/* DLWP_GRAPH_WIDE_ACT_NONE, DLWP_GRAPH_ACT_RELU or DLWP_GRAPH_ACT_SILU; res [rows][N] nullable.  der (nullable, SiLU */
/* only) receives the derivative rows d = s (1 + v (1 - s)).                                                          */
int dlwp_graph_wide_linear_fwd(const dlwp_graph_wide_operand* op, const float* w, const float* b, const float* res, float* y,
                               float* der, int N, int act, void* stream);
/* y = LayerNorm(z) gamma + beta [+ res] over rows of width C (biased variance, one wave per row); xhat [rows][C] and  */
/* rstd [rows] (both or neither) receive the normalised rows and 1 / sigma for dlwp_graph_wide_ln_bwd.                */
int dlwp_graph_wide_ln_fwd(const float* z, const float* gamma, const float* beta, const float* res, float* y, float* xhat,
                           float* rstd, long long rows, int C, float eps, void* stream);
/* WRITES dz [rows][C]; ggamma / gbeta (each nullable) are ACCUMULATED into from per-workgroup column sums folded in   */
/* workgroup order.  ws: dlwp_graph_wide_ln_bwd_ws_floats floats.                                                     */
long long dlwp_graph_wide_ln_bwd_ws_floats(long long rows, int C);
int dlwp_graph_wide_ln_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dz, float* ws,
                           float* ggamma, float* gbeta, long long rows, int C, void* stream);
/* gw [N][K] += dz^T . A, gb [N] += column sums of dz (NULL: none), A gathered as in the forward.  ws: scratch of      */
/* dlwp_graph_wide_wgrad0_ws_floats(op, N) floats (per-workgroup partial sums, folded in a fixed order).  A later      */
/* Linear's operand is stored rows: dlwp_conv1x1_wgrad takes them at any width.                                       */
long long dlwp_graph_wide_wgrad0_ws_floats(const dlwp_graph_wide_operand* op, int N);
int dlwp_graph_wide_wgrad0(const dlwp_graph_wide_operand* op, const float* dz, float* ws, float* gw, float* gb, int N,
                           void* stream);
/* dA = dz [rows][N] . w [N][K], WRITTEN in parts (each nullable except rows' out0):                                  */
/*   rows  out0 = dx [rows][D0], times mul [rows][D0] (nullable; mask != 0: kept where mul > 0, else zero -- ReLU's    */
/*         mask from the stored post-activation rows), + res                                                          */
/*   edge  out0 = de [B E][D0] (+ res), out1 = per-edge d_src [B E][D1], out2 = per-edge d_dst [B E][D2]               */
/*   node  out0 = d_agg [B Nd][D0], out1 = dv [B Nd][D1] (+ res)                                                       */
int dlwp_graph_wide_dgrad(const dlwp_graph_wide_operand* op, const float* dz, const float* w, const float* res, const float* mul,
                          int mask, float* out0, float* out1, float* out2, int N, void* stream);
/* out[b N + i] = [add[b N + i]] + sum_j in[b E + eid[j]] (ptr[i] <= j < ptr[i+1], in list order; mean != 0: divided   */
/* by the count), rows of width C, onto ONE node set of N nodes: the forward aggregation (in-CSR, Nd), and dv of an    */
/* edge block as two launches (out-CSR of d_src onto the Ns sources, in-CSR of d_dst onto the Nd destinations).        */
int dlwp_graph_wide_gather_sum(const float* in, const int* ptr, const int* eid, int mean, const float* add, float* out, int B,
                               int N, int E, int C, void* stream);
/* out[b E + k] = [add[b E + k]] + in[b N + dst[k]] (in_ptr != NULL: divided by the in-degree of dst[k]).              */
int dlwp_graph_wide_edge_gather(const float* in, const int* dst, const int* in_ptr, const float* add, float* out, int B, int N,
                                int E, int C, void* stream);

/* ---- training batches assembled on the device from resident datasets (csrc/batch_ops.hip, docs/kernels/data.md).        */
/* One launch per batch on the caller's stream; pure data movement (no atomics, no LDS), so two calls give the same bits.  */
/* A table row whose sample or window lies outside the resident data writes nothing for that row and reads nothing.        */
/* noise > 0 adds noise * z with z from the library's own counter-based stream (Philox4x32-10, counter                     */
/* (e >> 2, item, epoch, tag), key = the two halves of seed): the noise of a sample depends on (seed, epoch, item, element */
/* e inside the sample) only, never on the batch.  noise == 0 copies (or normalises) exactly and draws nothing.            */
#define DLWP_BATCH_TAG_NS 0x6e73u /* Philox counter word 3 of dlwp_ns_batch */
#define DLWP_BATCH_TAG_WB 0x7762u /* ... of dlwp_wb_batch */
/* u [N][T][F] (F = D H W floats per frame); table [B][2] int32 (sample i, crop start r);                                  */
/* x [B][L-1][F] = u[i][r .. r+L-2] (+ noise z), y [B][L-1][F] = u[i][r+1 .. r+L-1]; every source frame is read once.      */
int dlwp_ns_batch(const float* u, int N, int T, long long F, const int* table, int B, int L, float noise,
                  unsigned long long seed, int epoch, float* x, float* y, void* stream);
typedef struct {
    const float* base; /* [n_time][P] series, or [P] for a constant */
    float mean, std;
    int normalize;     /* != 0: (a - mean) / std in fp32, correctly rounded */
} dlwp_wb_channel;
/* chan: DEVICE array of nC constants, then nP prescribed, then nG prognostic channels; items [B] int32, t0 = item * L.    */
/* constants [B][1][nC][P]; prescribed [B][L][nP][P] from frames t0 .. t0+L-1; prognostic [B][L][nG][P] from the same      */
/* frames (+ noise z); target [B][L-context][nG][P] from frames t0+1+context .. t0+L.  The outputs of a group without      */
/* channels may be NULL and are not written.  An item is valid while 0 <= item and t0 + L + 1 <= n_time.                   */
int dlwp_wb_batch(const dlwp_wb_channel* chan, int nC, int nP, int nG, const int* items, int B, int L, int context, int n_time,
                  long long P, float noise, unsigned long long seed, int epoch, float* constants, float* prescribed,
                  float* prognostic, float* target, void* stream);

/* ---- the Navier-Stokes data generator's point-wise kernels (csrc/ns_solver.hip, docs/kernels/data.md "Navier-Stokes    */
/* generator"; reference: generate_ns_2d.py:27-130 and random_fields.py:8-64 as nsdata.py restates them).  Complex arrays    */
/* are interleaved fp32 pairs, 8-byte aligned; the state is the half spectrum [B][n][n/2+1] of an n x n field, n even and   */
/* >= 4.  Index a stands for the wavenumber a (a < n/2) or a - n, so the Nyquist row and column carry -n/2; k_x runs along   */
/* the rows, k_y along the columns.  lap = 4 pi^2 (k_x^2 + k_y^2) with lap[0][0] = 1.  No tables, no atomics, one writer    */
/* per output element: every launch gives the same bits, whatever the batch a sample travels in.                            */
#define DLWP_NS2D_TAG_GRF 0x6772u /* Philox counter word 3 of dlwp_ns2d_grf */
/* H [B][n][n/2+1]: half spectrum of the initial vorticity of the samples first_sample .. first_sample + B - 1.             */
/*   c[a][b] = sqrt_eig[a][b] (z[2 (a n + b)] + i z[2 (a n + b) + 1]),                                                       */
/*   sqrt_eig = n^2 sqrt(2) sigma (lap + tau^2)^(-alpha / 2), sqrt_eig[0][0] = 0 (here lap[0][0] = 0),                       */
/*   z[e] the normal of element e of the sample under counter (e >> 2, sample, 0, DLWP_NS2D_TAG_GRF), key = seed;           */
/*   H[a][b] = (c[a][b] + conj(c[(n - a) % n][(n - b) % n])) / 2, whose irfft2 (norm "backward") is Re(ifft2(c)).           */
int dlwp_ns2d_grf(unsigned long long seed, long long first_sample, int B, int n, float alpha, float tau, float sigma, float* H,
                  void* stream);
/* out [B][4][n][n/2+1] = i k_y psi, -i k_x psi, i k_x w, i k_y w with psi = w_h / lap and each k times 2 pi: the spectra    */
/* of the velocity components and the vorticity gradients, in the layout one channels-first dlwp_irfft2 reads.              */
int dlwp_ns2d_spectral_terms(const float* w_h, float* out, int B, int n, void* stream);
/* out [B][n][n] = q w_x + v w_y of fields [B][4][n][n] = (q, v, w_x, w_y).                                                  */
int dlwp_ns2d_advect(const float* fields, float* out, int B, int n, void* stream);
/* w_h <- (-dt D F_h + dt f_h + (1 - dt visc lap / 2) w_h) / (1 + dt visc lap / 2) in place, D = 1 where 3 |k_x| <= n and     */
/* 3 |k_y| <= n, else 0 (the 2/3 rule).  f_h is [n][n/2+1], or [B][n][n/2+1] when f_batched != 0.                            */
int dlwp_ns2d_cn_update(float* w_h, const float* F_h, const float* f_h, int f_batched, int B, int n, float dt, float visc,
                        void* stream);

/* bench probe: ONE forward `spatial` launch of an inner FNO block as the rollout issues it     */
/* (x = previous pre-activation, GELU on load; spec = [B][m1][m2c][C][2] mixed modes; fused      */
/* W-axis DFT of gelu(pre) into x1_out [B][H][m2c][C][2]).                                       */
int dlwp_fno_spatial_fwd_probe(const dlwp_fno_plan* plan, const float* x, const float* spec,
                               const float* wskip, const float* bias, float* pre, float* x1_out,
                               int B, void* stream);
/* bench probe: ONE forward per-mode launch (H-axis step of x1 [B][H][m2c][C][2] + the mode-truncated complex channel      */
/* contraction with wspec on the matrix cores) -> xhat, y [B][m1][m2c][C][2].                                               */
int dlwp_fno_mix_fwd_probe(const dlwp_fno_plan* plan, const float* x1, const float* wspec, float* xhat,
                           float* y, int B, void* stream);
/* debug: enqueue n dependent empty kernels of `blocks` workgroups (per-kernel floor probe)   */
int dlwp_debug_null_kernels(int n, int blocks, void* stream);
/* same with a body: every wave spins for `cycles` shader cycles; grid, block size and dynamic LDS chosen by the caller */
int dlwp_debug_spin_kernels(int n, int blocks, int threads, int cycles, int lds_bytes, void* stream);
/* debug: out[0] = shader-clock ticks, out[1] = 100 MHz ticks spent in a dependent-FMA loop   */
int dlwp_debug_clock_probe(unsigned long long* out, int iters, int blocks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DLWPMI_H */
