/*
 * vbnn_hip.h -- C ABI of the MI355X-native VBLinear hot path (libvbnn_hip.so).
 *
 * The reference (louissmit/VBNN) has no FFI of its own: its hot path is Lua calling
 * Torch7 tensor ops. Each entry point below therefore cites the Lua call site it
 * replaces (file:line under the reference tree). The host side that binds this ABI is
 *   - vbnn_amd/nn.py      (ctypes; same class/method names as VBLinear.lua / mlp.lua)
 *   - lua/VBLinear.lua    (LuaJIT FFI shim)
 *
 * Conventions
 *   - every function returns an int status (0 = VBNN_OK); the message of the last
 *     failure on the calling thread is vbnn_last_error(). No C++ exception crosses.
 *   - all tensor pointers are DEVICE pointers (hipMalloc'ed by anyone: this library's
 *     vbnn_buf_alloc, PyTorch-ROCm, ...). The library never retains them.
 *   - calls are asynchronous on the context's HIP stream; vbnn_sync / vbnn_buf_download
 *     are the only blocking calls.
 *   - matrices are dense row-major. "packed operands" are the GEMM-ready copies made by
 *     vbnn_pack: element type f32 or bf16 (dtype), leading dimension padded to a
 *     multiple of VBNN_KPAD elements with ZERO fill (allocate them zeroed). A packed bf16
 *     operand of 2^30 elements (rows x ld) or more is still computed, by the general kernel:
 *     the pipelined kernels address their operands with 32-bit byte offsets.
 *   - O = outputSize, I = inputSize, N = minibatch rows (local rows on this rank).
 */
#ifndef VBNN_HIP_H
#define VBNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)   /* the library is built with -fvisibility=hidden */
#endif

#define VBNN_ABI_VERSION 6
#define VBNN_KPAD 64            /* packed leading dimensions are multiples of this */

enum { VBNN_OK = 0, VBNN_ERR_INVALID = 1, VBNN_ERR_HIP = 2, VBNN_ERR_NOMEM = 3, VBNN_ERR_UNSUPPORTED = 4 };
enum { VBNN_F32 = 0, VBNN_BF16 = 1 };                       /* dtype of packed operands */
enum { VBNN_PACK_COPY = 0, VBNN_PACK_EXP = 1, VBNN_PACK_SQUARE = 2, VBNN_PACK_MUL = 3,
       VBNN_PACK_RELU = 4, VBNN_PACK_RELU_SQUARE = 5 };

typedef struct vbnn_ctx vbnn_ctx;

int vbnn_abi_version(void);
const char* vbnn_last_error(void);

/* test / A-B hook, PROCESS-wide: WHICH of the library's kernels computes a GEMM -- every setting computes the same results to
 * rounding (the parity tests force each kernel through the same checks); nothing here changes what is computed. (r04: the keys
 * that switched timing-only or never-selected forms -- fake noise, the K-split launches -- left the library with those forms:
 * tools/lab/.) Kernel selection is a property of the build under test, not of a context: set it
 * before the contexts start launching, from one thread). VBNN_DEBUG_GEMM_KERNEL: 0 = pick by shape (default), 1 = always the general MFMA
 * kernel, 2 = the pipelined bf16 kernel whenever the operands allow it, 3 = its two-pass 256 x 256 variant
 * whenever the shape and outputs allow it (whole tiles, the fused configuration). */
#define VBNN_DEBUG_GEMM_KERNEL 0
#define VBNN_DEBUG_V2_SCHEDULE 1   /* pipelined kernel schedule: -1 = by tile (default), 0 = DMAs in a burst after the barrier,
                                      2 = interleaved with the MFMAs, 4 = alternating read / MFMA clusters, the workgroup's
                                      halves one cluster apart (8-wave tiles only; the same results whichever: gemm_v2.h) */
#define VBNN_DEBUG_V2_TILE 2       /* pipelined kernel block tile: 0 = by shape (default), 256 = 256 x 128, 128 = 128 x 128,
                                      64 = 128 x 128 with a 2-stage ring, two workgroups per CU */
#define VBNN_DEBUG_V3_MIN_K 4      /* shortest K for which shape selection picks the two-pass 256 x 256 kernel (default 704) */
#define VBNN_DEBUG_V2_PSPLIT 5     /* pipelined kernel pair split (the pair's two GEMMs in different workgroups, parameter
                                      gradients only): -1 = by shape (default), 0 = never, 1 = whenever possible */
#define VBNN_DEBUG_V3_SPLIT 8      /* two-pass kernel's pair-split half-height launch for few-tile parameter gradients: -1 = by shape (default), 0 = never, 1 = whenever possible */
#define VBNN_DEBUG_V0 9            /* fp32 shapes of the launch-bound geometry: 1 = the latency kernel (gemm_v0.h; default), 0 = gemm_v1's 32 x 32 tile */
#define VBNN_DEBUG_HEAD_BACKWARD 10   /* the fused head's backward (vbnn_head_backward, bf16): -1 = by shape (default: the streaming form for whole
                                         128-unit x 32-row tiles with a separate finish kernel), 0 = the tile form, 1 = the streaming form
                                         whenever the operands allow it (also at sizes whose partial sums the tile form finishes in-launch) */
#define VBNN_DEBUG_KMAJOR 6        /* K-major operands (gemm_v3.h AK / BK): 1 = use when the shape allows (default), 0 = never, 2 = gemm_v3 only */
#define VBNN_DEBUG_V3_FOLD_SERIAL 12  /* the two-pass kernel's LRT forward, the noise fold between its passes: 0 = the software-pipelined
                                         form (default), 1 = the serial form, one quad at a time (additive; the same bits either way) */
int vbnn_debug_set(int key, int value);
/* The read side of the hook (additive, ABI 6). VBNN_DEBUG_LAST_HEAD_FORM: which form of the classifier head the LAST head call
 * of this process launched (vbnn_head_forward, vbnn_head_forward_slots, vbnn_head_backward, vbnn_head_forward_backward;
 * PROCESS-wide and host-side: written where the launch is chosen, nothing on the device), 0 before the first. A call that is
 * two launches (vbnn_head_forward_backward outside its one-launch sizes) leaves the form of its second, the backward. The value:
 *   bits 0-3   the entry: VBNN_HEAD_ENTRY_FORWARD (k_head_forward), _SLOTS (k_head_from_slots), _STEP (the one-launch
 *              forward + backward), _TILE (the 64 x 64 tile backward), _STREAM (the streaming backward)
 *   bit  4     the operand type: 0 = f32, 1 = bf16
 *   bit  5     VEC  (tile backward: 16-byte accesses)      bit 6   FULL (tile backward: whole tiles, no bounds checks)
 *   bits 8-15  CP   (tile backward: classes of the final weight kept in registers, 12 or 0)
 *   bits 16-17 the finish of the row-chunk partial sums: VBNN_HEAD_FINISH_NONE (a forward, or no sum asked for),
 *              _INLINE (the last arriver of the launch), _KERNEL (k_head_backward_finish follows)
 * Any key but this one, VBNN_DEBUG_LAST_GEMM_FORM and VBNN_DEBUG_LAST_CHAINED (below): -1. Nothing here changes what is launched. */
#define VBNN_DEBUG_LAST_HEAD_FORM 11
#define VBNN_HEAD_ENTRY_FORWARD 1
#define VBNN_HEAD_ENTRY_SLOTS 2
#define VBNN_HEAD_ENTRY_STEP 3
#define VBNN_HEAD_ENTRY_TILE 4
#define VBNN_HEAD_ENTRY_STREAM 5
#define VBNN_HEAD_FINISH_NONE 0
#define VBNN_HEAD_FINISH_INLINE 1
#define VBNN_HEAD_FINISH_KERNEL 2
#define VBNN_HEAD_FORM(entry, bf16, vec, full, cp, finish) ((entry) | ((bf16) << 4) | ((vec) << 5) | ((full) << 6) | ((cp) << 8) | ((finish) << 16))
/* VBNN_DEBUG_LAST_GEMM_FORM (additive, ABI 6): which GEMM launch the LAST call of vbnn_forward, vbnn_grad_input,
 * vbnn_acc_grad_parameters or vbnn_backward_pair chose in this process -- PROCESS-wide and host-side, written by the launcher where
 * it has picked its kernel (after every return that launches nothing; a launcher that answers VBNN_ERR_UNSUPPORTED and lets its
 * caller fall back leaves the value alone), 0 before the first. vbnn_backward_pair outside its one-launch sizes leaves the form of
 * its second call, gradInput. Nothing on the device, and nothing that selects a kernel, reads it. The value:
 *   bits 0-3   the kernel: VBNN_GEMM_KERNEL_V0 (the latency kernel, gemm_v0.h), _V0_PAIR (its backward-pair launch), _V1 (the
 *              general kernel, gemm_v1.h), _V1_PAIR, _V2 (the pipelined kernel, gemm_v2.h), _V3 (the two-pass 256 x 256 kernel,
 *              gemm_v3.h), _V3_SPLIT (its half-height pair-split launch)
 *   bits 4-5   the tile. V0 / V0_PAIR: 0 = 16 x 16 (narrow), 1 = 16 x 32 (wide; the pair: of its gradInput problem). V1: 0 = 32 x 32,
 *              1 = 64 x 64, 2 = 128 x 128. V2: 0 = 256 x 128, 1 = 128 x 128, 2 = 128 x 128 with the two-stage ring (two workgroups
 *              per CU). Else 0.
 *   bits 6-7   V2: the schedule / 2 (VBNN_DEBUG_V2_SCHEDULE 0, 2, 4 -> 0, 1, 2) after the tile's own limit. Else 0.
 *   bit  8     DUAL: both accumulators of the LRT pair in one workgroup (0: one accumulator per workgroup)
 *   bit  9     the pair split (V2, V3_SPLIT): the pair's two GEMMs in different workgroups of one grid
 *   bits 10-11 the `part` handed to the functor (vbnn_dw_args.part: 0, 1, 2)
 *   bit  12    A K-major        bit 13   B K-major   (0: K-contiguous, the packed form)
 *   bits 14-15 SQ: 1 = B2 = B . B, 2 = A2 = A . A formed in registers (fp32), 0 = both squares given
 *   bit  16    the row of ones (gradBias) synthesised by the kernel (fp32 K-major); 0 = stored in the operand, or none
 *   bit  17    the operand type: 0 = f32, 1 = bf16
 *   bit  18    fast_ok() of the epilogue functor at launch: whole tiles take the fast protocol, the others the guarded one
 *              (the pair launches: of both functors)
 *   bit  19    V3: the forward's fold between the passes in its serial form (VBNN_DEBUG_V3_FOLD_SERIAL)
 *   bits 20-21 the family: VBNN_GEMM_CLASS_FWD, _DX, _DW (the pair launches: _DW, whose DUAL and row of ones they record) */
#define VBNN_DEBUG_LAST_GEMM_FORM 13
#define VBNN_GEMM_KERNEL_V0 1
#define VBNN_GEMM_KERNEL_V0_PAIR 2
#define VBNN_GEMM_KERNEL_V1 3
#define VBNN_GEMM_KERNEL_V1_PAIR 4
#define VBNN_GEMM_KERNEL_V2 5
#define VBNN_GEMM_KERNEL_V3 6
#define VBNN_GEMM_KERNEL_V3_SPLIT 7
#define VBNN_GEMM_CLASS_FWD 1
#define VBNN_GEMM_CLASS_DX 2
#define VBNN_GEMM_CLASS_DW 3
#define VBNN_GEMM_FORM(kernel, tile, sched, dual, psplit, part, ak, bk, sq, ones, bf16, fast, serial, cls)                        \
    ((kernel) | ((tile) << 4) | ((sched) << 6) | ((dual) << 8) | ((psplit) << 9) | ((part) << 10) | ((ak) << 12) | ((bk) << 13) | \
     ((sq) << 14) | ((ones) << 16) | ((bf16) << 17) | ((fast) << 18) | ((serial) << 19) | ((cls) << 20))
int vbnn_debug_get(int key);

/* 1 when a GEMM with an M x N output and contraction length K would take the K-major form of the two-pass kernel
 * under the current selection (whole 256 x 256 tiles filling the CUs, K a multiple of 64, bf16): the host asks once
 * per layer whether it needs the transposed copies at all (accGradParameters: M = I, N = O, K = minibatch rows;
 * gradInput: M = I, N = minibatch rows, K = O). For accGradParameters the answer presumes the fused total-gradient form
 * with the operand shadows (vbnn_dw_args.grad_mu / grad_lv + mu_s / var_s): that is the only K-major epilogue. */
int vbnn_kmajor_supported(int64_t M, int64_t N, int64_t K);
/* The same question for accGradParameters of an I -> O layer on N rows, which has a second K-major form (the pair-split
 * launch for outputs with few tiles). bias_row = 1: the bias gradient is to come from the GEMM (vbnn_dw_args.gradBias),
 * K-major that means column I of x is all ones (and ld_x > I). Returns 0 (no: pass xT / gT), 1 (yes) or 2: yes, on the
 * two-pass kernel's pair-split + split-K launch, which reads x and x.x in whole 256-column tiles -- allocate them with
 * ld_x >= the row length (ones column included) rounded up to a multiple of 256, zero filled past the data; with a
 * smaller ld_x the call still works, on the slower launch. */
int vbnn_kmajor_supported_dw(int64_t I, int64_t O, int64_t N, int bias_row);
/* The same two questions for the launches of ONE context: a context made by vbnn_ctx_create_cu_budget tiles for its budget, every
 * other context (and the two calls above) for the whole device -- the plan is a property of the context, not of the process. */
int vbnn_ctx_kmajor_supported(vbnn_ctx* ctx, int64_t M, int64_t N, int64_t K);
int vbnn_ctx_kmajor_supported_dw(vbnn_ctx* ctx, int64_t I, int64_t O, int64_t N, int bias_row);

/* context = (device, stream). hip_stream is a hipStream_t; NULL = the device's default stream
 * (which is also what PyTorch-ROCm's default stream is, so the two stay ordered). */
int vbnn_ctx_create(int device, void* hip_stream, vbnn_ctx** out);
/* The same with a stream of the library's own that may only use `n_cus` of the device's compute units
 * (hipExtStreamCreateWithCUMask; the enabled units are spread evenly over the XCDs): the CU budget of the compute stream in
 * a data-parallel run, where RCCL's channels hold some units for the whole step -- a 256-tile GEMM launched on all 256
 * units then finishes the displaced tiles as a straggling second round, while a launch planned for the units it really
 * has (vbnn_ctx_kmajor_supported* and the shape heuristics of THIS context's calls read the budget) tiles for them. n_cus <= 0 or >= the device's
 * count: no mask, just an own stream. vbnn_ctx_stream returns the hipStream_t for hosts that enqueue their own work
 * (PyTorch: torch.cuda.ExternalStream). */
int vbnn_ctx_create_cu_budget(int device, int n_cus, vbnn_ctx** out);
int vbnn_ctx_stream(vbnn_ctx* ctx, void** hip_stream_out, int* n_cus_out);
int vbnn_ctx_destroy(vbnn_ctx* ctx);
int vbnn_ctx_set_stream(vbnn_ctx* ctx, void* hip_stream);
int vbnn_sync(vbnn_ctx* ctx);

/* device-buffer helpers for hosts without a tensor library on the device (the Lua shim;
 * replaces the cutorch :cuda() copies at VBLinear.lua:40-44,56-58 and main.lua:22-25). */
int vbnn_buf_alloc(vbnn_ctx* ctx, size_t bytes, void** dptr);   /* zero-initialised */
int vbnn_buf_free(vbnn_ctx* ctx, void* dptr);
int vbnn_buf_zero(vbnn_ctx* ctx, void* dptr, size_t bytes);
int vbnn_buf_upload(vbnn_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int vbnn_buf_download(vbnn_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);  /* blocks */

/* rows x cols standard normals (include/vbnn_philox.h contract):
 * out[r][c] = lane c&3 of vbnn_normal4(seed, stream, layer, draw, row0 + r, c >> 2), times `scale`.
 * Replaces randomkit.normal at VBLinear.lua:26-28 (means init) and mlp.lua:53 (He init);
 * also the synthetic-input generator of bench.py.
 * Held by tests/test_sweeps_gpu.py: out[r][c] is bit for bit fl(z scale), ONE fp32 multiply of the contract's normal; the row
 * word of the counter is (uint32_t)(row0 + r), so rows wrap at 2^32. Elements c >= cols of a row (the pitch's pads) are never
 * written. `out` / `ld` may be anything: 16-byte stores when out is 16-byte aligned and ld % 4 == 0, scalar stores otherwise. */
int vbnn_fill_normal(vbnn_ctx* ctx, float* out, int64_t rows, int64_t cols, int64_t ld,
                     uint64_t seed, uint32_t stream, uint32_t layer, uint32_t draw, int64_t row0,
                     float scale);
/* The same normals in the form the bf16 forward draws them: the same Philox words, Box-Muller on them by the hardware's
 * log2 / sqrt / sin / cos instead of the contract's bit-exact polynomial forms (csrc/common.h, vbnn_normal4_hw): equal to
 * vbnn_fill_normal's to a few 1e-7 absolute, a quarter of the instructions. The fp32 path (held sample for sample against the
 * oracle) draws the exact form; this entry exists so that a host or a test can see exactly what a bf16 forward used.
 * Held to |out - z scale| <= 2e-6 |scale| + 2^-24 |z scale| against the contract's z; pads and alignment as vbnn_fill_normal. */
int vbnn_fill_normal_hw(vbnn_ctx* ctx, float* out, int64_t rows, int64_t cols, int64_t ld,
                        uint64_t seed, uint32_t stream, uint32_t layer, uint32_t draw, int64_t row0,
                        float scale);

/* Both forms of the contract's Box-Muller (include/vbnn_philox.h, vbnn_box_muller) on GIVEN Philox words x0[i], x1[i] (device
 * arrays of n words): z_exact[2i], z_exact[2i + 1] = the bit-exact form (what the fp32 path and the oracle draw), z_hw[..] = the
 * hardware-transcendental form the bf16 forward draws. A diagnostic for hosts and tests: it is how the hardware form's distance
 * from the contract is pinned over ALL 2^24 radii and ALL 2^24 angles (tests/test_parity_gpu.py, tests/golden/normals_hw_error.json). */
int vbnn_box_muller_forms(vbnn_ctx* ctx, const uint32_t* x0, const uint32_t* x1, float* z_exact, float* z_hw, int64_t n);

/* VBLinear:compute_prior (VBLinear.lua:77-88). One fused sweep over means/lvars:
 *   stats[0] = sum(exp(lvars) + means^2)   (so var_hat = stats[0] / W, :86)
 *   stats[1] = sum(lvars)
 *   stats[2] = var_hat (as double)  -- read by later kernels on the device, no host sync
 * Optional caches (NULL to skip), exactly the reference's: vars (:78), stdv (:79), mu_sqe (:82).
 * `stats` is a device array of 4 doubles; stats[3] = W.
 * Held by tests/test_sweeps_gpu.py. Op for op in fp32 (no contraction): v = expf(l) (within 2 ulp of the exact exponential: the
 * one figure that is bounded, not bitwise), stdv = sqrtf(v) (the correctly rounded root of the stored vars), mu_sqe = fl(m m);
 * a term of stats[0] is fl(v + fl(m m)) widened to double; the sums are double, in an order that is fixed for a given W, and are
 * held to 1e-10 of the sum of their terms' magnitudes; stats[2] = (1 / W) stats[0] in double. means, lvars and the three caches
 * take 16-byte accesses when ALL that are given are 16-byte aligned, and 4-byte accesses otherwise (any float alignment works). */
int vbnn_compute_prior(vbnn_ctx* ctx, const float* means, const float* lvars, int64_t W,
                       float* vars, float* stdv, float* mu_sqe, double* stats);

/* VBLinear:sample (VBLinear.lua:49-64): weight = means + stdv (.) e, e ~ N(0,1) of shape O x I
 * regenerated from the Philox counter (stream EPS). e_out may be NULL (the reference keeps
 * self.e; the kernels never need it stored). stdv == NULL: use exp(lvars/2) of `lvars`.
 * Held by tests/test_sweeps_gpu.py: e_out is the contract's normal of (seed, EPS, layer, draw, row o, quad i >> 2) bit for bit;
 * weight = fl(means + fl(sd e)), two fp32 roundings, bit for bit when stdv is given; without it sd = sqrtf(expf(lvars)), expf
 * within 2 ulp. The five pointers take 16-byte accesses when I % 4 == 0 and all that are given are 16-byte aligned, 4-byte
 * accesses otherwise. */
int vbnn_wn_sample(vbnn_ctx* ctx, const float* means, const float* stdv, const float* lvars,
                   float* weight, float* e_out, int64_t O, int64_t I,
                   uint64_t seed, uint32_t layer, uint32_t draw);

/* Generic packer: dst[r][c] = T(f(src[r][c])) for r < rows, c < cols, with
 *   f = COPY | EXP | SQUARE | MUL (src * src2) | RELU | RELU_SQUARE;
 * dst is rows x ld_dst, dstT (optional) is the transpose, cols x ld_dstT. Pads are not
 * written (keep them zero). Produces every GEMM operand of the module-level path:
 * mu/sigma^2 shadows, x and x.x, g and g.r.
 * Held by tests/test_sweeps_gpu.py, every function x dtype x {dst, dstT, both}: COPY, MUL, RELU are T(fl(f)) bit for bit; SQUARE
 * and RELU_SQUARE square the value AFTER rounding it to T (T(fl(T(h)^2)), what the GEMM epilogues produce); EXP is expf, within
 * 2 ulp before the rounding to T. dstT holds the very values of dst. RELU is fmaxf(a, 0): a NaN gives +0 (RELU_SQUARE: +0), and
 * -0.0 gives +0 (IEEE 754 leaves that sign open; gfx950's maximum orders -0 below +0), as vbnn_relu_forward. Accesses are element-wise:
 * src, ld_src and both outputs may have any alignment and pitch; elements c >= cols of a dst row and r >= rows of a dstT row
 * are never written. */
int vbnn_pack(vbnn_ctx* ctx, int dtype, int func, const float* src, const float* src2, int64_t ld_src,
              int64_t rows, int64_t cols, void* dst, int64_t ld_dst, void* dstT, int64_t ld_dstT);

/* ---- the three GEMM families of the layer (MFMA kernels, fused epilogues) ------------------- */

typedef struct vbnn_fwd_args {
    /* operands (packed, dtype): A = weights-side O x ld_w, B = input-side N x ld_x */
    const void* w;      /* mu shadow (LRT) or sampled-weight shadow (WN / MAP)            */
    const void* w2;     /* sigma^2 shadow, LRT only (NULL: single GEMM)                    */
    const void* x;      /* input                                                           */
    const void* x2;     /* input squared, LRT only. dtype F32: may be NULL -- the kernel forms x.x in  */
                        /* registers while staging x (bit for bit what the packer would store)  */
    int64_t ld_w, ld_x;
    int64_t N, I, O;
    const float* bias;  /* O, may be NULL                                                  */
    /* LRT noise: z[n][o] from (seed, ZETA, layer, draw, row0 + n, o >> 2); ignored if w2 == NULL */
    uint64_t seed; uint32_t layer; uint32_t draw; int64_t row0;
    /* outputs, each optional */
    float* y;  int64_t ld_y;        /* pre-activation output (the module's `output`), N x O     */
    void* r;  int64_t ld_r;         /* z / (2 sqrt(v)), saved for backward (LRT), N x ld_r:      */
    int r_packed;                   /* 0: float (the module path); 1: element type = dtype       */
    int relu;                       /* apply ReLU before writing the packed outputs below        */
    void* h;  void* h2;  int64_t ld_h;     /* next layer's packed input and its square, N x ld_h  */
    void* hT; void* h2T; int64_t ld_hT;    /* their transposes, O x ld_hT                         */
    /* > 0: the N rows are SEVERAL Monte-Carlo draws of one minibatch stacked (main.lua:32-37's S loop as rows): row n is
     * minibatch row n % rows_per_draw of draw `draw + n / rows_per_draw`, and its noise is addressed accordingly -- bit
     * for bit the z of that draw's own launch. The backward GEMMs then sum over all draws in one pass (K = N). 0: off. */
    int64_t rows_per_draw;
    /* optional DEVICE-RESIDENT draw counter (NULL: off): the noise is addressed by draw + *draw_dev, read when the kernel
     * runs -- so that a step whose launches were captured into a graph (vbnn_capture_*) draws fresh noise at every replay:
     * the host's `sample()` is then vbnn_sample (a device-side increment, itself a node of the graph) and `draw` stays a
     * constant base. General kernel only: with it set the pipelined bf16 kernels are not selected (the launch-bound
     * configurations are the ones worth capturing; the others take the counter as the launch argument above). */
    const uint32_t* draw_dev;
    /* optional (NULL: off; ABI 5): the logits of the classifier head that follows the LAST VB layer (mlp.lua:29: the final
     * nn.Linear, C <= 16 outputs) formed by THIS launch, from its output tiles while they are still in registers: every
     * 256 x 256 tile adds nothing to memory traffic but 2 x 256 rows x 16 fp32 partial logits, written to the fixed slot
     * head_slots[2 tile + half][n][16] (n_slots = vbnn_forward_head_slots(...) slots of N x 16 floats; classes >= head_C are
     * undefined), and the head (vbnn_head_forward_slots / vbnn_head_args.logit_slots) adds the slots in order instead of
     * re-reading h: bitwise reproducible, no atomics. head_w3: the final weight PACKED (head_C x head_ld_w, dtype), as
     * vbnn_prepare / vbnn_update leave it. Only where vbnn_forward_head_slots says so (> 0); elsewhere the call fails. */
    const void* head_w3; int64_t head_ld_w; int64_t head_C; float* head_slots;
} vbnn_fwd_args;

/* updateOutput. WN/MAP: y = x w^T + b  (inherited nn.Linear:updateOutput, VBLinear.lua:7).
 * LRT: m = x mu^T + b, v = (x.x)(sigma^2)^T, y = m + sqrt(v) . z   (north_star).
 * dtype F32 (the general kernel): `x` may be the RAW minibatch -- any 16-byte-aligned row-major matrix with ld_x >= I,
 * ld_x % 4 == 0, columns [I, ld_x) finite; the K walk is masked at the row end, no zero padding is needed -- so an fp32
 * host needs no vbnn_pack_input at all. */
int vbnn_forward(vbnn_ctx* ctx, int dtype, const vbnn_fwd_args* a);
/* How many slots the forward of an I -> O layer on N rows writes when given vbnn_fwd_args.head_slots for a C-class head, under
 * this context's kernel selection: 0 = that launch cannot carry the head's logits (use vbnn_head_forward on h), otherwise
 * allocate n x N x 16 floats. (bf16 layers whose forward runs on the two-pass 256 x 256 kernel: 2 slots per 256 output units.) */
int vbnn_forward_head_slots(vbnn_ctx* ctx, int dtype, int64_t N, int64_t I, int64_t O, int64_t C);

typedef struct vbnn_dx_args {
    /* A = transposed weights-side I x ld_wT, B = gradient-side N x ld_g */
    const void* wT;     /* mu^T shadow (LRT) or sampled-weight^T shadow (WN)               */
    const void* w2T;    /* (sigma^2)^T shadow, LRT only                                     */
    const void* g;      /* dL/dy packed                                                     */
    const void* gv;     /* dL/dv = g . r packed, LRT only                                   */
    int64_t ld_wT, ld_g;
    int64_t N, I, O;
    const void* x; int64_t ld_x;    /* this layer's packed input (LRT term 2 x . (gv sigma^2);  */
                                    /* also the ReLU mask of the previous module)               */
    float* gx; int64_t ld_gx;       /* gradInput N x I f32, optional                            */
    /* optional fused hand-off to the previous VB layer: g_prev = gx . [x > 0], gv_prev = g_prev . r_prev */
    int relu_mask;
    const void* r_prev; int64_t ld_r_prev; int r_prev_packed;   /* the previous layer's `r`, same typing rule */
    void* g_prev; void* gv_prev; int64_t ld_gp;      /* N x ld_gp   */
    void* gT_prev; void* gvT_prev; int64_t ld_gpT;   /* I x ld_gpT  */
    /* optional K-MAJOR weights: mu, sigma^2 as the forward holds them (O x ld_w). When vbnn_kmajor_supported(I, N, O)
     * says so the GEMM reads these and wT / w2T may be NULL: the parameter sweep writes no transposed shadows.
     * dtype F32: always (any shape) -- with wT == NULL the general kernel reads w / w2 K-major. */
    const void* w; const void* w2; int64_t ld_w;
} vbnn_dx_args;

/* updateGradInput. WN: gradInput = g w (inherited, VBLinear.lua:109-110).
 * LRT: gradInput = g mu + 2 x . (gv sigma^2). */
int vbnn_grad_input(vbnn_ctx* ctx, int dtype, const vbnn_dx_args* a);

typedef struct vbnn_dw_args {
    /* A = input-side transposed I x ld_n, B = gradient-side transposed O x ld_n (K = N rows) */
    const void* xT;     /* x^T                                                              */
    const void* x2T;    /* (x.x)^T, LRT only                                                */
    const void* gT;     /* g^T                                                              */
    const void* gvT;    /* gv^T, LRT only                                                   */
    int64_t ld_n;
    int64_t N, I, O;
    float scale;        /* accGradParameters' scale (applied to gradWeight only, as the reference) */
    int accumulate;     /* 1: += (Torch semantics); 0: overwrite (first draw after resetAcc)  */
    float* gradWeight;  /* O x I, += scale * g^T x                      (VBLinear.lua:113)     */
    float* gradSum;     /* O x I. WN:  += (g^T x) . e                    (VBLinear.lua:114-115) */
                        /*        LRT: += 2 (gv^T x.x) . stdv   (same units)    */
    /* WN: e regenerated from (seed, EPS, layer, draw). LRT: stdv = exp(lvars / 2). */
    uint64_t seed; uint32_t layer; uint32_t draw;
    const float* lvars;
    /* optional fused total-gradient outputs (likelihood/S + kl_scale * KL gradient),
     * VBLinear.lua:90-98 folded into the epilogue; NULL to skip. Needs means, lvars, stats. */
    float* grad_mu; float* grad_lv;
    const float* means; const double* stats; float B; float S; float kl_scale;
    /* optional: the bias gradient from the same GEMM. xT (and x2T) then have I + 1 rows, row I of xT all ones (row I
     * of x2T anything finite): output row I of the first GEMM is sum_n g[n][o], written as
     * gradBias[o] (+)= scale * that -- what vbnn_acc_grad_bias(g) gives, without another pass over g. NULL: off. */
    float* gradBias;
    /* optional K-MAJOR operands: the untransposed x, x.x (N x ld_x) and g, gv (N x ld_g) exactly as the forward and
     * gradInput GEMMs hold them. When vbnn_kmajor_supported(I, O, N) says so the GEMM reads these (transpose reads in
     * LDS) and xT / x2T / gT / gvT may be NULL: no epilogue has to write transposed copies. Otherwise xT.. are used.
     * dtype F32: always (any shape, part = 0) -- with xT == NULL the general kernel reads x and g (gv) K-major; x2 may
     * then be NULL (x.x is formed in registers), x may be the raw minibatch (ld_x % 4 == 0), and gradBias needs no row or
     * column of ones anywhere: the kernel synthesises it. */
    const void* x; const void* x2; const void* g; const void* gv; int64_t ld_x; int64_t ld_g;
    /* optional (fused total gradients only, dtype BF16): the packed operand shadows mu_s, var_s = exp(lvars) (O x ld_w,
     * as vbnn_prepare / vbnn_update leave them). When given, the epilogue reads mu and sigma^2 FROM THEM -- 4 B per weight
     * instead of 8, and no exp -- i.e. d/dlvars = (gv^T x.x) . s2 + KL'(s2), d/dmeans = g^T x + KL'(mu) with s2, mu the
     * values the forward GEMMs multiplied by (bf16-rounded); means / lvars are then not read -- except by gradSum (and the
     * weight-noise d/dlvars), whose stdv stays exp(lvars / 2) of the fp32 parameter when the same call asks for it. NULL: fp32
     * means / lvars.
     * REQUIRED by the K-major launches (x / g given, xT / gT NULL): their epilogue reads the shadows only, so a caller that
     * passes K-major operands without mu_s / var_s gets VBNN_ERR_INVALID -- keep the transposed operands for that case. */
    const void* mu_s; const void* var_s; int64_t ld_w;
    /* 0 (default): both GEMMs of the LRT pair, every output. 1: only the first GEMM (g^T x) and what depends on it
     * (gradWeight / grad_mu, gradBias); 2: only the second (gv^T x.x) and what depends on it (gradSum / grad_lv). Calling
     * with part = 2 and then part = 1 gives bit for bit the outputs of part = 0 (each output depends on ONE accumulator)
     * as two launches -- so that a data-parallel host can start the exchange of the finished d/dlvars while the d/dmeans
     * GEMM still runs (vbnn_allreduce_grads between the two calls). LRT pairs only. */
    int part;
    const uint32_t* draw_dev;   /* as vbnn_fwd_args.draw_dev (the weight-noise form regenerates e from the counter) */
} vbnn_dw_args;

/* accGradParameters (VBLinear.lua:112-118), one GEMM instead of the reference's two. */
int vbnn_acc_grad_parameters(vbnn_ctx* ctx, int dtype, const vbnn_dw_args* a);

/* accGradParameters AND updateGradInput of one layer in one call: both consume that layer's gradOutput and neither reads
 * what the other writes (nn.Sequential:backward runs them back to back, mlp.lua:79). Where one launch can carry both -- dtype
 * F32 with the K-major operand forms, at the launch-bound tile geometry (BASELINE configs[1]: a launch there is 10 us of
 * latency chain with the chip a fraction busy) -- it does, each tile computed exactly as by its own launch (bitwise the same
 * outputs); everywhere else this IS the two calls, accGradParameters first. */
int vbnn_backward_pair(vbnn_ctx* ctx, int dtype, const vbnn_dx_args* dx, const vbnn_dw_args* dw);

/* The same two calls for the bf16 layers whose two gradients each run on the two-pass 256 x 256 kernel (additive, ABI 6). Where
 * dtype is BF16 and BOTH blocks would on their own take that kernel's plain K-major LRT form (whole 256 x 256 tiles that fill the
 * device, part = 0, accumulate = 0, no gradBias row, no transposed outputs, the fast / folded epilogue protocols), ONE launch
 * carries both: workgroup t computes tile t of the first problem, issues its stores and goes straight on to tile t of the second,
 * so the first tile's stores drain under the second tile's matrix passes. No workgroup waits for another; every tile is computed
 * exactly as by its own launch (bitwise the same outputs). Everywhere else this IS the two calls. `order` says which problem
 * comes first, in the one launch and in the two calls alike. VBNN_DEBUG_LAST_GEMM_FORM reads as after the two calls;
 * vbnn_debug_get(VBNN_DEBUG_LAST_CHAINED) is 1 if the last call of this process went out as one launch, else 0;
 * vbnn_debug_set(VBNN_DEBUG_CHAIN_OFF, 1) makes every call the two calls (A/B, tests). */
#define VBNN_CHAIN_DX_FIRST 0
#define VBNN_CHAIN_DW_FIRST 1
#define VBNN_DEBUG_LAST_CHAINED 15
#define VBNN_DEBUG_CHAIN_OFF 16
int vbnn_backward_chain(vbnn_ctx* ctx, int dtype, const vbnn_dx_args* dx, const vbnn_dw_args* dw, int order);

/* gradBias += scale * sum_n g[n][o]  (the parent call at VBLinear.lua:113). g is N x ld_g of
 * `dtype` (F32: the module's gradOutput; BF16: a packed operand of the fused path). */
int vbnn_acc_grad_bias(vbnn_ctx* ctx, int dtype, const void* g, int64_t ld_g, int64_t N, int64_t O,
                       float scale, int accumulate, float* gradBias);

/* Per-step parameter sweep of the fused path: one read of means/lvars writes the packed GEMM
 * shadows mu_s, var_s = exp(lvars) (O x ld_w) and, if asked, their transposes (I x ld_wT), and the
 * statistics of VBLinear:compute_prior (VBLinear.lua:77-88) into stats[0..3] as vbnn_compute_prior.
 * Held by tests/test_sweeps_gpu.py (this entry and vbnn_prepare, which leave the same bits): mu_s = T(means) bit for bit;
 * var_s = T(expf(lvars)), expf within 2 ulp; the transposes hold the very values of the row-major shadows; the statistics as
 * vbnn_compute_prior states them, whichever form the sweep takes (64 x 64 tiles, or flat when no transposes are asked for).
 * ALIGNMENT. mu_s / var_s are written with 4-element vector stores unconditionally: their bases must be 16-byte aligned and
 * ld_w a multiple of 4 elements (the convention is VBNN_KPAD). muT_s / varT_s take vector stores when ld_wT % 4 == 0 (their
 * bases aligned likewise) and element stores otherwise. means / lvars take 16-byte loads when I % 4 == 0 and both are 16-byte
 * aligned, 4-byte loads otherwise. Pad elements (c >= I of a shadow row, r >= O of a transposed row) are never written. */
int vbnn_prep_layer(vbnn_ctx* ctx, int dtype, const float* means, const float* lvars, int64_t O, int64_t I,
                    void* mu_s, void* var_s, int64_t ld_w, void* muT_s, void* varT_s, int64_t ld_wT,
                    double* stats);

/* The same sweep for every VB layer of a model in ONE call (n_layers <= 8), plus optionally the plain packing of one
 * more small f32 matrix (the final nn.Linear's weight, mlp.lua:29: dst rows x ld_dst and its transpose cols x
 * ld_dstT, either may be NULL): one sweep kernel per layer and a single finish kernel for all the statistics and the
 * extra matrix -- two launches fewer per step than n_layers x vbnn_prep_layer + vbnn_pack.
 * Each layer is held to vbnn_prep_layer's contract (alignment included) and its four statistics are its own. The extra matrix
 * is T(src) bit for bit in dst and in dstT, each with its own pitch, stored element-wise (any alignment); pads are not written. */
typedef struct vbnn_prep_desc {
    const float* means; const float* lvars; int64_t O, I;
    void* mu_s; void* var_s; int64_t ld_w;
    void* muT_s; void* varT_s; int64_t ld_wT;      /* NULL / 0: no transposed shadows */
    double* stats;
} vbnn_prep_desc;
typedef struct vbnn_pack_desc {
    const float* src; int64_t rows, cols, ld_src;
    void* dst; int64_t ld_dst; void* dstT; int64_t ld_dstT;
} vbnn_pack_desc;
int vbnn_prepare(vbnn_ctx* ctx, int dtype, int n_layers, const vbnn_prep_desc* layers, const vbnn_pack_desc* extra);

/* ---- KL ("LC") terms ------------------------------------------------------------------------ */

/* VBLinear:compute_mugrads (VBLinear.lua:90-93): gradWeight /= S in place; lcg = means / (B var_hat).
 * VBLinear:compute_vargrads (:95-98): gradSum = gradSum / (2S) . stdv in place;
 *                                      lcg = ((-1/vars + 1/var_hat) / (2B)) . vars.
 * var_hat is read from stats[2] on the device. vars/stdv NULL: derived from lvars.
 * Held by tests/test_sweeps_gpu.py, bit for bit, in this fp32 order: den = (float)((double) B stats[2]); lcg = means / den;
 * gradWeight = gradWeight / S.  inv_vh = (float)(1.0 / stats[2]); a = -(1 / v) + inv_vh; lcg = (a / (2 B)) v;
 * gradSum = (gradSum / (2 S)) stdv. Without vars / stdv: v = expf(lvars) (within 2 ulp), stdv = sqrtf(v). Either output may
 * be NULL. Accesses are 4-byte: any float alignment. */
int vbnn_compute_mugrads(vbnn_ctx* ctx, const float* means, const double* stats, float B, float S,
                         float* gradWeight, float* lcg, int64_t W);
int vbnn_compute_vargrads(vbnn_ctx* ctx, const float* lvars, const float* vars, const float* stdv,
                          const double* stats, float B, float S, float* gradSum, float* lcg, int64_t W);

/* VBLinear:calc_lc (VBLinear.lua:99-103) with the :sum() of mlp.lua:112 fused:
 * lc_sum_dev[0] = sum_w [log sqrt(var_hat) - log sqrt(vars) + (mu_sqe + vars - var_hat) / (2 var_hat)] / B.
 * lc_elem (optional) receives the per-weight tensor the Lua method returns.
 * vars / mu_sqe: the caches of the last compute_prior (the reference reads exactly those, so its
 * LC is one optimiser step stale, main.lua:174-177); NULL: derive from means / lvars.
 * Held by tests/test_sweeps_gpu.py. Per weight, in fp32: first = -logf(sqrtf(v)) + (float) log(sqrt(var_hat));
 * second = (q + (v - (float) var_hat)) / (2 (float) var_hat); lc = (first + second) (1 / B) -- within an ABSOLUTE bound derived
 * from these roundings (tests/_sweeps_np.py), meaningful where the halves cancel (a fresh layer). The sum is the double sum of
 * those very fp32 elements (to 1e-10 of their magnitudes) and the same bits with and without lc_elem. 4-byte accesses. */
int vbnn_calc_lc(vbnn_ctx* ctx, const float* means, const float* lvars, const float* vars, const float* mu_sqe,
                 const double* stats, float B, float* lc_elem, double* lc_sum_dev, int64_t W);

/* The minibatch (N x I f32, row pitch ld_src) as GEMM operands in one pass: x_s, x2_s = (rounded x)^2 (N x ld_x)
 * and their transposes (I x ld_xT); x2_s / xT_s / x2T_s optional. Replaces the host->device copies of
 * main.lua:22-25 plus two vbnn_pack calls. rows_per_draw > 0 (vbnn_fwd_args.rows_per_draw): the N operand rows are several
 * Monte-Carlo draws of ONE minibatch of rows_per_draw rows -- operand row n is src row n % rows_per_draw, so the host never
 * materialises the S-fold input. 0: off.
 * Held by tests/test_sweeps_gpu.py, bit for bit: x_s = T(x), x2_s = T(fl(T(x)^2)) (the square of the ROUNDED x), and the
 * transposes hold the very values of the row-major outputs. ALIGNMENT. x_s / x2_s are written with 4-element vector stores
 * unconditionally: bases 16-byte aligned, ld_x a multiple of 4 (checked; the convention is VBNN_KPAD). xT_s / x2T_s take vector
 * stores when ld_xT % 4 == 0 (bases aligned likewise), element stores otherwise. src takes 16-byte loads when it is 16-byte
 * aligned and ld_src % 4 == 0, 4-byte loads otherwise. Pad elements are never written. */
int vbnn_pack_input(vbnn_ctx* ctx, int dtype, const float* src, int64_t ld_src, int64_t N, int64_t I, void* x_s,
                    void* x2_s, int64_t ld_x, void* xT_s, void* x2T_s, int64_t ld_xT, int64_t rows_per_draw);

/* ---- the update that follows the hot path -------------------------------- */

/* optim.adam as VBLinear:update calls it on means / lvars (VBLinear.lua:135-143), one streaming pass:
 *   g = grad (+ grad2);  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g.g;
 *   x -= lr sqrt(1 - b2^t) / (1 - b1^t) . m / (sqrt(v) + eps)
 * grad2 (optional) is added to grad first (the torch.add of likelihood and KL parts, VBLinear.lua:131-134);
 * lambda < 1 selects the early torch/optim variant's decay b1_t = b1 lambda^(t-1) (config.lua:52,56,61), 1 = off;
 * t is state.t after its increment (>= 1). norms_dev (optional, 2 doubles): { |update|, |x_new| }, the two norms of
 * the reference's `mu_normratio = torch.norm(update) / torch.norm(x)` (VBLinear.lua:139,144).
 * optim is not vendored by the reference and its version is unpinned: this is the published algorithm. */
int vbnn_adam_step(vbnn_ctx* ctx, float* x, const float* grad, const float* grad2, float* m, float* v, int64_t n,
                   float lr, float beta1, float beta2, float eps, float lambda, int64_t t, double* norms_dev);
/* optim.sgd with only learningRate set (config.lua:51-54): x -= lr * grad (VBLinear.lua:125-128, mlp.lua:120-128). */
int vbnn_sgd_step(vbnn_ctx* ctx, float* x, const float* grad, int64_t n, float lr);

/* VBLinear:update (VBLinear.lua:124-166) for every VB layer of a model in ONE call, fused with what the NEXT minibatch
 * needs: per layer one sweep applies optim.sgd to the bias (:125-128) and optim.adam to means and lvars (:135-143, the
 * arithmetic of vbnn_adam_step) from the TOTAL gradients (likelihood / S + KL: what the fused accGradParameters
 * epilogue leaves in grad_mu / grad_lv, i.e. `mugrad` / `vgrad` of :132,134) and, from the NEW parameters in the same
 * pass, writes the packed GEMM shadows and the prior statistics exactly as vbnn_prepare would (the reference runs
 * compute_prior inside update as well, :130) -- so a training step needs no separate parameter sweep. `extra` as in
 * vbnn_prepare (the final nn.Linear's weight, packed after its own vbnn_sgd_step). One finish kernel for all layers.
 * log14 (optional, 14 doubles per layer) receives the series VBLinear.lua:149-164 logs, in that order:
 *   vlc grad, vle grad, mlc grad, mle grad (norm of the KL / likelihood part over norm of the updated parameter; the
 *   KL parts are re-derived from the pre-update parameters and stats[2], the likelihood parts are total - KL),
 *   min / max / mean variance (updated), var hat (pre-update, as self.var_hat is at :156), mean / std (unbiased) / min /
 *   max of the updated means, mu normratio, var normratio (:139,144).
 * stats must hold the statistics of the PRE-update parameters on entry (vbnn_prepare / the previous vbnn_update). */
typedef struct vbnn_adam_cfg { float lr, beta1, beta2, eps, lambda; int64_t t; } vbnn_adam_cfg;
typedef struct vbnn_update_desc {
    float* means; float* lvars; int64_t O, I;          /* updated in place */
    void* mu_s; void* var_s; int64_t ld_w;             /* shadows of the NEW parameters (as vbnn_prep_desc) */
    void* muT_s; void* varT_s; int64_t ld_wT;          /* NULL / 0: no transposed shadows */
    double* stats;                                     /* in: pre-update statistics; out: statistics of the new parameters */
    const float* grad_mu; const float* grad_lv;        /* total gradients, O x I */
    float* m_mu; float* v_mu; float* m_lv; float* v_lv;    /* Adam state, O x I each */
    vbnn_adam_cfg mu, lv;                              /* opt.meanState / opt.varState (config.lua:55-64) */
    float* bias; const float* grad_bias; float lr_bias;    /* optional (NULL): optim.sgd on the bias */
    float B;                                           /* opt.B: scale of the KL parts in the logged norms */
    double* log14;                                     /* optional */
    /* 0 (default): grad_mu / grad_lv are the TOTAL gradients (the accGradParameters epilogue added the KL part, from the
     * bf16 operand shadows in the fused bf16 configuration). > 0: they are the likelihood parts alone (the host passed
     * vbnn_dw_args.kl_scale = 0) and the sweep adds kl_add x the KL gradient itself, from the fp32 means / lvars and stats[2]
     * (VBLinear.lua:91,96 exactly as the reference computes them) -- the exact form: the shadow form's (bf16(s2) / var_hat - 1)
     * cancels to ~2^-9 absolute. Data-parallel: 1 on every rank (the all-reduced likelihood sum + the KL gradient once). */
    float kl_add;
} vbnn_update_desc;
int vbnn_update(vbnn_ctx* ctx, int dtype, int n_layers, const vbnn_update_desc* layers, const vbnn_pack_desc* extra);

/* ---- training under a held pruning mask (additive, ABI 6): the two parameter sweeps and the KL sum of the network that
 * signal-to-noise pruning (below) leaves. The reference only counts what would go (mainviz.lua:20-27); it never trains on what
 * is left. A mask is the byte tensor vbnn_prune_pack writes: O x I uint8_t, non-zero = pruned. `masks` is a HOST array of
 * n_layers device pointers, a NULL entry = that layer is unmasked; masks == NULL or every entry NULL: the call IS vbnn_prepare /
 * vbnn_update. The forward and both backward GEMMs read the operand shadows only, so with +0 in a pruned weight's shadow entries
 * every GEMM of the step computes the pruned network; nothing else of the step changes. Per weight of a masked layer:
 *   kept (mask 0)    exactly the arithmetic of vbnn_prepare / vbnn_update (one kernel definition, a template flag);
 *   pruned           means, lvars and the four Adam moments keep their bits (the weight is frozen, not zeroed: dropping the mask
 *                    brings it back); mu_s, var_s and, where asked for, muT_s, varT_s receive +0; it enters none of the sums,
 *                    none of the 14 logged series, no min / max. Its values never reach the arithmetic; where the unmasked sweep
 *                    loads four weights as one 16-byte vector, a group with at least one kept weight is still loaded whole and
 *                    the pruned lanes are dropped, a group without one is not loaded. Stores touch kept weights only.
 * Statistics of a masked layer: stats[0] = sum over KEPT of (exp(lvars) + means^2), stats[1] = sum over kept of lvars, stats[3] =
 * n_kept (where W stands), stats[2] = stats[0] / n_kept: the prior variance of the network that exists, which is what the KL term of
 * the accGradParameters epilogue, kl_add and vbnn_calc_lc_masked then read. log14's means and unbiased std divide by n_kept. n_kept
 * is counted in the sweep (integer-valued doubles in the fixed partial order: two runs give the same bits). A mask that prunes
 * NOTHING gives the unmasked call's bits in every output (stats[2] then as vbnn_prepare forms it, (1 / W) x stats[0]); a layer
 * with no kept weight gets stats[0..3] = 0, +0 shadows and no log14. The bias step, `extra` and the Adam step sizes are untouched.
 * vbnn_update_masked: `stats` must hold the MASKED statistics of the pre-update parameters on entry. */
int vbnn_prepare_masked(vbnn_ctx* ctx, int dtype, int n_layers, const vbnn_prep_desc* layers,
                        const uint8_t* const* masks, const vbnn_pack_desc* extra);
int vbnn_update_masked(vbnn_ctx* ctx, int dtype, int n_layers, const vbnn_update_desc* layers,
                       const uint8_t* const* masks, const vbnn_pack_desc* extra);
/* vbnn_calc_lc (from means / lvars, no caches) with the pruned weights left out of the sum and written as 0 in lc_elem; `stats`
 * as the masked sweeps leave them. mask == NULL: vbnn_calc_lc. */
int vbnn_calc_lc_masked(vbnn_ctx* ctx, const float* means, const float* lvars, const uint8_t* mask,
                        const double* stats, float B, float* lc_elem, double* lc_sum_dev, int64_t W);

/* ---- data-parallel exchange (north_star: "RCCL all-reduce over xGMI on the (mu, log sigma^2) gradients after
 * accGradParameters"; the reference itself is single-device, main.lua:142 sets BLAS threads only) ------------------
 * One process per GPU, one communicator per process. Rank 0 calls vbnn_comm_unique_id and the HOST side hands the
 * VBNN_COMM_ID_BYTES to every rank by its own means (a file, a socket, torch.distributed's store, MPI ...); every
 * rank then calls vbnn_comm_create (collective: it returns when all `world` ranks have joined).
 * vbnn_allreduce_grads(buf, n): in-place SUM over ranks of n floats -- a layer's contiguous gradient bucket
 * [d/dmeans | d/dlvars | d/dbias]. It is ordered after everything enqueued so far on the context's stream (the
 * accGradParameters that fills the bucket) and runs on the communicator's own high-priority stream, i.e. beside
 * the launches that follow (the rest of backward). Every rank must issue the same sequence of calls.
 * vbnn_comm_finish: orders the context's stream behind every exchange issued so far (no host wait; follow with
 * vbnn_sync to block). The criterion already divides by the GLOBAL batch and the fused KL gradient carries
 * 1 / world (vbnn_dw_args.kl_scale), so the sum IS the gradient: no division afterwards.
 * librccl is loaded on first use (dlopen: VBNN_RCCL_PATH, then librccl.so.1); without it these calls return
 * VBNN_ERR_UNSUPPORTED and nothing else in the library is affected. (r05: the ordering behind the context's stream is a TRIGGER word --
 * a one-thread kernel on the context's stream, a one-wave kernel polling it on the exchange stream in front of the collective -- not
 * an event: a marker packet costs the context's stream ~8 us of bubble per bucket; vbnn_comm_finish hands BACK the same way, the roles
 * swapped, as vbnn_p2p_finish does; VBNN_COMM_FLAG_TRIGGER=0 / VBNN_P2P_FLAG_TRIGGER=0 at create keep the events.) */
#define VBNN_COMM_ID_BYTES 128
typedef struct vbnn_comm vbnn_comm;
int vbnn_comm_unique_id(void* id_out /* VBNN_COMM_ID_BYTES, host memory */);
int vbnn_comm_create(vbnn_ctx* ctx, int rank, int world, const void* id, vbnn_comm** out);
int vbnn_comm_destroy(vbnn_comm* comm);
int vbnn_comm_info(vbnn_comm* comm, int* rank, int* world, int* ranks_in_comm /* as RCCL counts them */);
int vbnn_allreduce_grads(vbnn_comm* comm, float* buf, int64_t n);
int vbnn_comm_finish(vbnn_comm* comm);
/* OPTIONAL half-size exchange (160.1 MB fp32 / 80.1 MB bf16 per step of the wide configuration): the
 * same call on a bf16 copy of the bucket, with vbnn_cast_grads to make it and to widen the sum back. The default exchange
 * is fp32; this one rounds every rank's contribution to bf16 (RNE) and lets RCCL sum in bf16 -- a different gradient
 * (relative 2^-9 per element and hop), for hosts that want the exchange hidden more than the last bits.
 * vbnn_cast_grads(to_bf16 = 1): dst[i] = bf16(src[i]), src fp32; (0): dst[i] = float(src[i]), src bf16; on the context's stream. */
int vbnn_allreduce_grads_bf16(vbnn_comm* comm, void* buf_bf16, int64_t n);
int vbnn_cast_grads(vbnn_ctx* ctx, int to_bf16, const void* src, void* dst, int64_t n);
/* all_dev[r] = rank r's *mine_dev (device memory, 8 bytes per rank), gathered over the same communicator and stream:
 * lets the host verify that `world` distinct processes / devices take part in the exchange. */
int vbnn_comm_allgather_u64(vbnn_comm* comm, const uint64_t* mine_dev, uint64_t* all_dev);
/* The two halves of the all-reduce as calls of their own, for the SHARDED-UPDATE exchange (an option beside north_star's
 * all-reduce; engine.py: opt.exchange_mode = "sharded"): after accGradParameters the gradient regions are
 * reduce-SCATTERED (rank r ends with the fp32 sums of its 1 / world of every layer's rows), rank r runs vbnn_update on that slice
 * alone (Adam state and fp32 master parameters sharded), and what is all-GATHERED afterwards is the packed operand shadows the
 * next forward reads -- bf16 mu and sigma^2, 4 bytes per weight instead of the 8 bytes of fp32 gradients an all-reduce's second
 * half moves -- plus four doubles of prior statistics per layer: 0.75x the bytes, 1 / world of the update sweep, fp32 sums.
 * Both are in place, ordered behind the context's stream, run on the exchange stream (vbnn_comm_finish orders the context's
 * stream behind them). reduce_scatter: buf holds world x n_per_rank floats; afterwards floats [rank n_per_rank, (rank + 1)
 * n_per_rank) are the sums over ranks (the rest is undefined). all_gather: buf holds world x bytes_per_rank bytes, rank r
 * contributes bytes [r bytes_per_rank, (r + 1) bytes_per_rank). */
int vbnn_comm_reduce_scatter(vbnn_comm* comm, float* buf, int64_t n_per_rank);
int vbnn_comm_all_gather(vbnn_comm* comm, void* buf, int64_t bytes_per_rank);
/* Device-side glue of that exchange. vbnn_stats_combine: parts = [world][n_layers][4] doubles, rank r's block being the `stats`
 * its slice's vbnn_update left (sum(exp(lvars) + means^2), sum(lvars), -, slice weights), gathered over the ranks; writes each
 * layer's statistics of the WHOLE layer (sums in rank order; var_hat as vbnn_update forms it) into stats[l]. Every rank computes
 * the same doubles. vbnn_transpose_packed: dst[c][r] = src[r][c] for a packed operand -- layers that keep transposed shadows
 * rebuild them from the gathered mu_s / var_s. */
int vbnn_stats_combine(vbnn_ctx* ctx, int n_layers, int world, const double* parts, double* const* stats);
int vbnn_transpose_packed(vbnn_ctx* ctx, int dtype, const void* src, int64_t ld_src, int64_t rows, int64_t cols, void* dst, int64_t ld_dst);

/* ---- the same exchange WITHOUT a collective library: direct reduce-scatter + all-gather over peer-mapped arenas
 * (vbnn_amd/csrc/p2p.hip; SURVEY.md section 5's fallback should RCCL put the 160 MB all-reduce on a single ring: every GPU of an
 * 8-GPU node has seven point-to-point xGMI links, and this form moves an eighth of the bucket over each of them at once).
 * vbnn_p2p_create allocates THE gradient arena of this rank (arena_floats fp32, zeroed: the host keeps its gradients there, as
 * engine.py's flat arena) and returns its device pointer and this rank's VBNN_P2P_HANDLE_BYTES handle; the host passes the
 * handles round by its own means (as the RCCL unique id), every rank calls vbnn_p2p_connect with all of them in rank order
 * (world x VBNN_P2P_HANDLE_BYTES), and from then on vbnn_p2p_allreduce(offset, n) sums arena[offset, offset + n) over the ranks
 * in place: ordered behind the context's stream, run on a high-priority stream of its own, the sum formed in rank order (bitwise
 * the same arena on every rank). vbnn_p2p_finish orders the context's stream behind it -- and launches the ONE exit barrier of the
 * exchanges issued since the last finish ("every rank has finished gathering": only then may the arena be overwritten), so a host
 * calls it before it lets anything write the arena again. Every rank issues the same sequence. (r05: a bucket is handed from the
 * context's stream to the exchange stream through a TRIGGER word of the rank's flag page -- a one-thread kernel behind the launch
 * that fills the bucket, polled by the exchange's first barrier -- not through an event: a marker packet costs the compute stream
 * ~8 us of bubble per bucket and the exchange stream ~12 us to wake up; VBNN_P2P_FLAG_TRIGGER=0 at create keeps the events.)
 * A barrier whose peers never arrive gives up after a bounded WALL time -- 20 s by default, VBNN_P2P_TIMEOUT_S in the environment
 * at create, or vbnn_p2p_set_timeout -- instead of hanging the device, and raises the exchange's status word: from then on every
 * data kernel of the exchange is a no-op (the arena keeps this rank's OWN gradients; no partial sum is ever written over them)
 * and later barriers signal without polling; the rank also marks itself dead in every PEER's flag page, so each peer's next barrier
 * fails at once and its data kernels stop too -- within one barrier no rank believes a sum that a stopped rank took no part in.
 * vbnn_p2p_status (blocking on the exchange stream) reports the epoch of the barrier
 * that failed: the host checks it before it lets an update read the arena (engine.py: FusedMLP.update / check_exchange) and,
 * having re-synchronised the ranks by its own means, may re-arm the exchange with vbnn_p2p_clear_status. The host runs one
 * barrier of its own between vbnn_p2p_connect and the first exchange (comm.P2PExchange). At most 8 ranks (one node); peers on
 * other devices need peer access (xGMI / PCIe P2P). */
#define VBNN_P2P_HANDLE_BYTES 128
typedef struct vbnn_p2p vbnn_p2p;
int vbnn_p2p_create(vbnn_ctx* ctx, int rank, int world, size_t arena_floats, vbnn_p2p** out, void** arena_out, void* handle_out);
int vbnn_p2p_connect(vbnn_p2p* p, const void* all_handles);
int vbnn_p2p_allreduce(vbnn_p2p* p, size_t offset_floats, int64_t n);
int vbnn_p2p_finish(vbnn_p2p* p);
/* the same two halves over the peer-mapped arena (regions of the arena, in floats; equal chunks, rank r's at offset + r x
 * n_per_rank): whatever the sharded-update exchange gathers -- the operand shadows, the statistics -- lives IN the arena then
 * (the host allocates it large enough and places them there) */
int vbnn_p2p_reduce_scatter(vbnn_p2p* p, size_t offset_floats, int64_t n_per_rank);
int vbnn_p2p_all_gather(vbnn_p2p* p, size_t offset_floats, int64_t n_per_rank);
int vbnn_p2p_status(vbnn_p2p* p, int* rank, int* world, unsigned* gave_up);
int vbnn_p2p_set_timeout(vbnn_p2p* p, double seconds);
int vbnn_p2p_clear_status(vbnn_p2p* p);
int vbnn_p2p_destroy(vbnn_p2p* p);
/* (ABI 6) The data kernels are built to CO-RESIDE with the GEMM launches they overlap -- no LDS, at most 48 VGPRs (what two
 * 226-register GEMM waves leave of a SIMD's file), `world` loads in flight per lane -- so their grids are small:
 * vbnn_p2p_set_grid(reduce-scatter workgroups, all-gather workgroups PER PEER; 0 = keep; defaults 256 and 32, or
 * VBNN_P2P_RS_BLOCKS / VBNN_P2P_AG_BLOCKS at create). vbnn_p2p_standin (LAB, world == 1 only): vbnn_p2p_allreduce then runs what one
 * rank of a sim_world-rank exchange runs -- same barriers, kernels, grids, stream, event -- against this arena standing in for its
 * peers', each phase paced to the wall time `inbound_GBps` of link bandwidth would need (0: unpaced): what the exchange costs the
 * launches beside it, priced on ONE GPU (tools/overlap_standin.py). The arena holds nothing meaningful afterwards. 0 switches off. */
int vbnn_p2p_set_grid(vbnn_p2p* p, int rs_blocks, int ag_blocks_per_peer);
int vbnn_p2p_standin(vbnn_p2p* p, int sim_world, double inbound_GBps);

/* ---- (ABI 6) what THIS device holds, measured in the run that reports a throughput (bench.py's `box` block) ------------------
 * The boxes of a pool differ by 5-7 % on one binary (the clock a power-bound chip holds); the reference's only timing hook is a
 * commented-out sys.clock() (main.lua:20). vbnn_box_calibrate runs two fixed probes on the context's stream and BLOCKS until
 * they are done (~70 ms; 1 GiB of scratch, freed again): a register-only MFMA loop on every SIMD (2 waves x 2^15
 * v_mfma_f32_16x16x32_bf16, live operands) -- mfma_clock_ghz = median over workgroups of d(s_memtime) / d(s_memrealtime) x 100 MHz,
 * mfma_tflops = its flops / its time -- and a 512 MiB -> 512 MiB copy: hbm_TBps (bytes read + written per second). */
typedef struct vbnn_box_info {
    double mfma_clock_ghz, mfma_tflops, mfma_ms;
    double hbm_TBps, hbm_ms;
    int64_t hbm_bytes;
    int cus, reserved;
} vbnn_box_info;
int vbnn_box_calibrate(vbnn_ctx* ctx, vbnn_box_info* out);

/* ---- a whole step as ONE graph launch (launch-bound configurations: BASELINE configs[1], the reference's own batch-1
 * S = 30 operating point, config.lua:11,32) ----------------------------------------------------------------------------
 * mlp:sample() (mlp.lua:69-74) on the device: *draw_dev += by, ordered on the context's stream like any launch. With
 * vbnn_fwd_args.draw_dev pointing at the same word, a captured step is replayable: every replay advances the counter
 * and draws the noise of ITS draw, exactly what the same calls issued one by one compute (tested bitwise). */
int vbnn_sample(vbnn_ctx* ctx, uint32_t* draw_dev, uint32_t by);
/* vbnn_capture_begin: from here on the context's launches are RECORDED, not run (hipStreamBeginCapture on its stream --
 * which must not be the NULL stream). Issue one step's calls as usual (every buffer already allocated, every kernel
 * launched at least once before: allocation and first-launch configuration cannot be captured), then vbnn_capture_end
 * returns the executable graph. vbnn_graph_launch replays it on that stream (asynchronous, like a launch); the arguments
 * -- pointers, sizes, the accumulate flags -- are the recorded ones, the data behind the pointers is read at replay time.
 * vbnn_graph_info: kernel nodes / all nodes of the graph. */
typedef struct vbnn_graph vbnn_graph;
int vbnn_capture_begin(vbnn_ctx* ctx);
int vbnn_capture_end(vbnn_ctx* ctx, vbnn_graph** out);
int vbnn_graph_launch(vbnn_graph* g);
int vbnn_graph_info(vbnn_graph* g, int* kernel_nodes, int* nodes);
int vbnn_graph_destroy(vbnn_graph* g);

/* ---- glue modules on the measured path (mlp.lua:12-32) --------------------------------------- */
int vbnn_relu_forward(vbnn_ctx* ctx, const float* x, float* y, int64_t n);
int vbnn_relu_backward(vbnn_ctx* ctx, const float* x, const float* g, float* gx, int64_t n);
/* nn.LogSoftMax + nn.ClassNLLCriterion (sizeAverage) fused, forward and backward in one pass:
 *   out = logsoftmax(logits); loss_sum_dev[0] += -sum_n out[n][t_n] * inv_n;
 *   correct_dev[0] += #rows whose arg-max equals the target (utils.lua:11-27);
 *   g_logits = (exp(out) - onehot) * inv_n     (= LogSoftMax:backward(ClassNLL:backward)).
 * inv_n = 1 / (global minibatch rows). Targets are 0-based int32. A target outside [0, C - 1] is clamped into it (a negative
 * one counts as class 0, one past the end as class C - 1) for the loss, the gradient and the hit count alike: such a row
 * is never read out of bounds and is never dropped. Of equal maxima the first (lowest class) is the arg-max. The launch's
 * loss is formed in double in a fixed order (block partials + one finish block, no float atomics) and then added to
 * loss_sum_dev[0]: bitwise reproducible. */
int vbnn_logsoftmax_nll(vbnn_ctx* ctx, const float* logits, int64_t ld, const int32_t* target,
                        int64_t N, int64_t C, float inv_n, float* out, float* g_logits,
                        double* loss_sum_dev, int32_t* correct_dev);

/* nn.MSECriterion (sizeAverage) on an N x D output, for BASELINE.json configs[4] ("synthetic 4096-dim regression"; the
 * reference itself only ever uses ClassNLL, mlp.lua:32): criterion:forward + :backward in ONE pass over y and target,
 *   loss_sum_dev[0] (+)= inv_nd * sum (y - t)^2;   g[n][d] = 2 inv_nd (y - t)   (g optional),
 * inv_nd = 1 / (GLOBAL rows x D). The sum is formed in a fixed order (block partials + one finish block: bitwise
 * reproducible); accumulate = 0 stores it, 1 adds to it (the S draws of a minibatch). vbnn_mse_backward: g alone. */
int vbnn_mse_forward(vbnn_ctx* ctx, const float* y, int64_t ld_y, const float* target, int64_t ld_t, int64_t N, int64_t D,
                     float inv_nd, float* g, int64_t ld_g, int accumulate, double* loss_sum_dev);
int vbnn_mse_backward(vbnn_ctx* ctx, const float* y, int64_t ld_y, const float* target, int64_t ld_t, int64_t N, int64_t D,
                      float inv_nd, float* g, int64_t ld_g);

/* The heteroscedastic Gaussian likelihood (additive, ABI 6; not in the reference): the final Linear has 2 D outputs per row,
 * columns [0, D) the mean m, columns [D, 2 D) s = the log of the noise variance; target is N x D. criterion:forward + :backward
 * in ONE pass over y and target, the shape of vbnn_mse_forward: ld_y >= 2 D, g is N x 2 D (ld_g >= 2 D; optional in the forward),
 * inv_nd = 1 / (GLOBAL rows x D). All element arithmetic is fp32, operation by operation as written (compiled without
 * floating-point contraction; expf is the library function, not the fast intrinsic). Per element, with s_min <= s_max:
 *   s_c = min(max(s, s_min), s_max) (a NaN s stays NaN);   w = expf(-s_c);   d = t - m;   e = 0.5f * (s_c + (d * d) * w)
 *   loss_sum_dev[0] (+)= inv_nd * sum e      -- the negative log density WITHOUT its constant 0.5 log(2 pi) per element;
 *   g_m = (inv_nd * (m - t)) * w;
 *   g_s = (0.5f * inv_nd) * (1 - (d * d) * w), and exactly +0 where s < s_min or s > s_max (the clamp has no slope there).
 * The sum is formed in double in a fixed order (block partials + one finish block, no float atomics: bitwise reproducible);
 * accumulate = 0 stores it, 1 adds to it. A NaN in y reaches the loss and the two gradient elements of its own (row, output),
 * and nothing else. vbnn_gauss_nll_backward: g alone, the same bits. */
int vbnn_gauss_nll_forward(vbnn_ctx* ctx, const float* y, int64_t ld_y, const float* target, int64_t ld_t, int64_t N, int64_t D,
                           float inv_nd, float s_min, float s_max, float* g, int64_t ld_g, int accumulate, double* loss_sum_dev);
int vbnn_gauss_nll_backward(vbnn_ctx* ctx, const float* y, int64_t ld_y, const float* target, int64_t ld_t, int64_t N, int64_t D,
                            float inv_nd, float s_min, float s_max, float* g, int64_t ld_g);

/* The Bernoulli likelihood (additive, ABI 6; not in the reference): D independent sigmoid outputs per row -- binary
 * classification with D = 1, multi-label classification with D labels. y holds the final Linear's N x D logits (ld_y >= D),
 * target is N x D fp32 in [0, 1] (0 / 1 labels; soft labels are allowed). criterion:forward + :backward in ONE pass over y and
 * target, the shape of vbnn_mse_forward: g is N x D (ld_g >= D; optional in the forward), inv_nd = 1 / (GLOBAL rows x D). Each
 * of the three streams takes the 16-byte or the scalar access path on its own leading dimension and base address. All element
 * arithmetic is fp32, operation by operation as written (compiled without floating-point contraction; expf and logf are the
 * library functions, the divisions are correctly rounded). Per element, z the logit and t the target:
 *   u = expf(-|z|);   w = 1 + u;   l1p = (logf(w) * u) / (w - 1)  (u itself where w == 1) -- log1p(u) in the moments family's
 *     form (vbnn_predict_class_moments below), not the library's log1pf;
 *   e = (fmaxf(z, 0) - z * t) + l1p          -- -[t log sigmoid(z) + (1 - t) log(1 - sigmoid(z))], stable for any finite z;
 *   sig = z >= 0 ? 1 / w : u / w;
 *   loss_sum_dev[0] (+)= inv_nd * sum e;     g = inv_nd * (sig - t).
 * The sum is formed in double in a fixed order (block partials + one finish block, no float atomics: bitwise reproducible);
 * accumulate = 0 stores it, 1 adds to it. correct_dev (optional, NULL to skip): the number of label hits, elements with
 * (z > 0) == (t > 0.5f), is ADDED to correct_dev[0] by an integer atomic -- exact for any grid; the caller zeroes it. A NaN logit
 * is a miss. Logits are finite or NaN; a NaN reaches the loss and its own gradient element, and nothing else.
 * vbnn_bce_backward: g alone, the same bits. */
int vbnn_bce_forward(vbnn_ctx* ctx, const float* y, int64_t ld_y, const float* target, int64_t ld_t, int64_t N, int64_t D,
                     float inv_nd, float* g, int64_t ld_g, int accumulate, double* loss_sum_dev, int32_t* correct_dev);
int vbnn_bce_backward(vbnn_ctx* ctx, const float* y, int64_t ld_y, const float* target, int64_t ld_t, int64_t N, int64_t D,
                      float inv_nd, float* g, int64_t ld_g);

/* mlp.lua:29-32 fused for a small class count (C <= 16): final nn.Linear + nn.LogSoftMax +
 * nn.ClassNLLCriterion as streaming kernels over the packed N x H activation `h` (dtype) and the packed
 * final weight `w3` (C x ld_w, dtype). Forward: logits = h w3^T + bias, out = logsoftmax,
 * g_logits = d(loss)/d(logits) (N x C f32); `logits`, `out` optional. The loss (sum of -out[n][target] * inv_n) and
 * the hit count are summed in a fixed order inside the launch (bitwise reproducible) and stored to loss_sum_dev[0]
 * / correct_dev[0] when accumulate = 0, added to them when accumulate = 1 (the S draws of a minibatch,
 * mlp.lua:76-84): no memset of the two accumulators is needed. rows_per_draw > 0: stacked draws, row n's target is
 * target[n % rows_per_draw] (`target` holds one minibatch's rows_per_draw entries). A target outside [0, C - 1] is clamped
 * into it for the loss, g_logits and the hit count, as in vbnn_logsoftmax_nll (the same holds for vbnn_head_forward_slots and
 * vbnn_head_forward_backward); of equal maxima the first is the arg-max. */
int vbnn_head_forward(vbnn_ctx* ctx, int dtype, const void* h, int64_t ld_h, const void* w3, int64_t ld_w,
                      const float* bias, const int32_t* target, int64_t N, int64_t H, int64_t C, float inv_n,
                      float* logits, float* out, float* g_logits, int accumulate, double* loss_sum_dev,
                      int32_t* correct_dev, int64_t rows_per_draw);
/* The same forward from partial logits a vbnn_forward launch left in `slots` (vbnn_fwd_args.head_slots: n_slots x N x 16
 * floats): logits[n][c] = bias[c] + slots[0][n][c] + slots[1][n][c] + ... in that order, then exactly vbnn_head_forward's
 * log-softmax, loss, hit count and g_logits. h is not read. */
int vbnn_head_forward_slots(vbnn_ctx* ctx, const float* slots, int64_t n_slots, const float* bias, const int32_t* target,
                            int64_t N, int64_t C, float inv_n, float* logits, float* out, float* g_logits, int accumulate,
                            double* loss_sum_dev, int32_t* correct_dev, int64_t rows_per_draw);
/* Backward of the same head in one pass over h: gradWeight (C x H) / gradBias (C) of the final Linear (accumulate
 * as in vbnn_acc_grad_parameters; NULL to skip), its gradInput pushed through the ReLU straight into the last VB
 * layer's packed gradient operands (same meaning as the hand-off fields of vbnn_dx_args), and optionally
 * gradBias_prev (H, f32): the column sums of g_prev as stored, i.e. what vbnn_acc_grad_bias(g_prev, scale 1) would
 * give -- the bias gradient of that VB layer (VBLinear.lua:112-113, parent.accGradParameters); NULL to skip. */
int vbnn_head_backward(vbnn_ctx* ctx, int dtype, const void* h, int64_t ld_h, const void* w3, int64_t ld_w,
                       const float* g_logits, int64_t N, int64_t H, int64_t C, int accumulate, float* gradWeight,
                       float* gradBias, float* gradBias_prev, int relu_mask, const void* r_prev, int64_t ld_r_prev,
                       int r_prev_packed, void* g_prev, void* gv_prev, int64_t ld_gp, void* gT_prev, void* gvT_prev,
                       int64_t ld_gpT);

/* mlp.lua:77-83 for the fused head in ONE call: model:forward's last three modules, criterion:forward / :backward and
 * model:backward's first three -- exactly vbnn_head_forward followed by vbnn_head_backward on the same arguments (the
 * fields below carry the names and meanings of those two calls' parameters). For fp32 at launch-bound sizes
 * (N x H <= 2^20, H even, no transposed copies asked for) it is ONE launch: every workgroup recomputes the logits of its 16
 * rows (same bits as vbnn_head_forward's) instead of waiting for a first kernel's g_logits, forms its 16 x 64 tile of the
 * gradInput and its rows' terms of gradWeight / gradBias / gradBias_prev, and the last workgroup of a column block adds the
 * partials in row order (bitwise reproducible; the sums are formed in a different order from vbnn_head_backward's, so
 * the two paths agree to rounding). Everywhere else the call IS the two launches. */
typedef struct vbnn_head_args {
    const void* h; int64_t ld_h;            /* packed N x ld_h input of the final Linear */
    const void* w3; int64_t ld_w;           /* packed C x ld_w weight */
    const float* bias;                      /* C, or NULL */
    const int32_t* target;                  /* rows_per_draw (stacked draws) or N entries */
    int64_t N, H, C;
    int64_t rows_per_draw;
    float inv_n;
    int32_t accumulate;                     /* of loss / hits and of the three gradients alike (the S draws of a minibatch) */
    float* logits; float* out; float* g_logits;         /* N x C each; logits, out optional */
    double* loss_sum_dev; int32_t* correct_dev;
    float* gradWeight; float* gradBias; float* gradBias_prev;   /* C x H, C, H; NULL to skip */
    int32_t relu_mask; int32_t r_prev_packed;
    const void* r_prev; int64_t ld_r_prev;
    void* g_prev; void* gv_prev; int64_t ld_gp;
    void* gT_prev; void* gvT_prev; int64_t ld_gpT;
    /* optional (ABI 5): the forward half from partial logits left by the last VB layer's forward (vbnn_fwd_args.head_slots):
     * as vbnn_head_forward_slots, then vbnn_head_backward. NULL / 0: the logits are computed from h. */
    const float* logit_slots; int64_t n_slots;
} vbnn_head_args;
int vbnn_head_forward_backward(vbnn_ctx* ctx, int dtype, const vbnn_head_args* a);

/* Posterior-predictive head (C <= 16): mlp:test's S draws (mlp.lua:86-107, main.lua:55-74) averaged as PROBABILITIES instead
 * of as per-draw criteria, with the per-example uncertainty the reference's author plots (visualize.lua:66-100,
 * show_uncertainties). Operand row n = s R + r is draw s of minibatch row r (the rows_per_draw = R layout of
 * vbnn_fwd_args). Per draw, in draw order: logits_s = h[n] w3^T + bias, bitwise vbnn_head_forward's on the same h;
 * o_s = log_softmax(logits_s) (first maximum wins, as Tensor:max); and per row a running state in fp32:
 *   L[c] = logsumexp over the draws so far of o_s[c] (online; never a sum of probabilities, which underflow),
 *   sum_s H(p_s) with H(p_s) = -sum_c exp(o_s[c]) o_s[c],  sum_s -o_s[t_r],  sum_s [argmax o_s = t_r].
 * The finish, per row: log p = L - log S, p = exp(log p), entropy = H[p], expected_entropy = sum_s H(p_s) / S,
 * mutual_info = entropy - expected_entropy (the epistemic part), pred = argmax p (first maximum).
 * Logits are finite or NaN. A NaN logit in any draw of a row (a NaN in h reaches every class of its row) makes every float
 * output of that row NaN -- probs, log_probs, entropy, expected_entropy, mutual_info -- and the float totals ([0] and [2]) NaN,
 * and leaves every other row bit for bit alone; the online logsumexp keeps a NaN, as vbnn_predict_class_moments' does. Such a
 * row is no hit in totals [1], its NaN draw none in [3]; its pred is unspecified but inside [0, C - 1]. */
enum { VBNN_PREDICT_STACKED = 0, VBNN_PREDICT_ACCUMULATE = 1 };
typedef struct vbnn_predict_args {
    const void* h; int64_t ld_h;            /* packed input of the final Linear (dtype): S x R rows (STACKED) or R rows (ACCUMULATE) */
    const void* w3; int64_t ld_w;           /* packed C x ld_w final weight, as vbnn_prepare / vbnn_update leave it */
    const float* bias;                      /* C, or NULL */
    const int32_t* target;                  /* R class indices, or NULL: no totals (targets are clamped to [0, C - 1]) */
    int64_t R;                              /* minibatch rows */
    int64_t H, C;                           /* hidden width (columns of h / w3 read), classes (1 .. 16) */
    int64_t S;                              /* draws of the WHOLE prediction (>= 1): the finish divides by it */
    /* VBNN_PREDICT_STACKED: h holds all S draws and this one call walks them in order (first / final / state ignored: the
     * state stays in registers). VBNN_PREDICT_ACCUMULATE: h holds ONE draw; the running state lives in `state` between
     * calls. Both forms run the same update in the same order: given the same h per draw, their outputs are bitwise equal. */
    int32_t form;
    int32_t first;                          /* ACCUMULATE: 1 = this draw starts the state (nothing is read from `state`) */
    int32_t final;                          /* ACCUMULATE: 1 = finish after this draw (the outputs and totals are written) */
    float* state;                           /* ACCUMULATE: R x (C + 3) floats, row r = { L[0 .. C-1], sum H, sum -o[t], hits } */
    /* outputs of the finish, each optional (NULL to skip) */
    float* probs; float* log_probs;         /* R x C: p(y | x, D) ~ 1/S sum_s softmax(f_s(x)), and its log */
    float* entropy;                         /* R: H[p] (total predictive uncertainty) */
    float* expected_entropy;                /* R: 1/S sum_s H(p_s) (the aleatoric part) */
    float* mutual_info;                     /* R: entropy - expected_entropy (the epistemic part) */
    int32_t* pred;                          /* R: argmax p */
    /* with target: 4 doubles, WRITTEN by the finish, each summed over rows in a fixed order inside the launch (bitwise
     * reproducible, no float atomics): { sum_r -log p[t_r], sum_r [pred = t_r], sum_{r,s} -o_s[t_r], sum_{r,s} hits } --
     * the predictive NLL, the ensemble's hits, and the reference's test metrics (mlp:test's mean criterion and accuracy
     * are the last two / (R S)). NULL to skip. */
    double* totals;
} vbnn_predict_args;
int vbnn_head_predict(vbnn_ctx* ctx, int dtype, const vbnn_predict_args* a);

/* Regression posterior predictive (additive, ABI 6): the moments over S draws of the final Linear's f32 outputs y_s (R x D per
 * draw) -- the predictive mean, the spread of the draws per output (the epistemic variance) -- and, with targets, the squared
 * errors and the log density of the equal-weight mixture of N(y_s, tau^2 I) at the target. All arithmetic is fp32, operation
 * by operation as written here (the file is compiled without floating-point contraction; divisions are correctly rounded).
 * Per element (r, d), from mean = M2 = 0, over the draws s = 0 .. S-1 in order (Welford):
 *   delta = y - mean;   mean = mean + delta / float(s + 1);   M2 = M2 + delta * (y - mean)
 * Finish per element: mean is stored as it stands; var = M2 / float(S) -- the variance of the mixture's components (S = 1
 * gives exactly 0, equal draws give exactly 0). The total predictive variance of an output is var + noise_var.
 * Per row and draw, with a target: e_s = sum_d (t - y_s)^2; sum_s e_s is kept as a running sum (draw 0 starts it); with
 * noise_var > 0 the running single-value online logsumexp L of a_s = -e_s * c, c = 0.5f / noise_var: draw 0 sets L = a_0,
 * every later draw L = max(L, a) + log1p(exp(-|L - a|)).
 * Finish per row: row_sq_err = sum_d (t - mean)^2;  row_var = (sum_d var) / float(D);
 *   row_log_lik = L - log(float(S)) - (0.5f * float(D)) * log(6.2831855f * noise_var).
 * Every row sum (e_s, row_sq_err, sum_d var) is formed in an order that depends on D alone: a row is worked by T = 64 threads
 * (D <= 256) or T = 256 (above); thread i adds, in ascending order, the columns 4 q .. 4 q + 3 of its quads q = i, i + T, ...;
 * the threads of a wave are added by the xor butterfly 32, 16, .. 1; the four waves in wave order. The same assignment holds
 * on the 16-byte and on the scalar access path (chosen per launch from D, the leading dimensions and the base addresses), in
 * both forms, for every R and row position. Pad columns are never read. A NaN in y reaches its element, its row's row values
 * and the totals, and no other row.
 * VBNN_MOMENTS_STACKED: y holds all S draws (draw s = rows [s R, (s+1) R)); one call walks them with the running moments in
 * registers (D <= VBNN_MOMENTS_STACKED_MAX_D; draw / state ignored). VBNN_MOMENTS_ACCUMULATE: y holds ONE draw, number `draw`;
 * the running values live in `state` between the S calls and every call rewrites it. Both forms run one device function per
 * draw: given the same y per draw, every output and total is bitwise equal between them. */
enum { VBNN_MOMENTS_STACKED = 0, VBNN_MOMENTS_ACCUMULATE = 1 };
#define VBNN_MOMENTS_STACKED_MAX_D 4096   /* largest D the STACKED form takes */
typedef struct vbnn_moments_args {
    const float* y; int64_t ld_y;       /* f32 outputs of the final Linear: S R x D (STACKED; draw s = rows [s R, (s+1) R)) or R x D (ACCUMULATE) */
    const float* target; int64_t ld_t;  /* R x D regression targets, or NULL */
    int64_t R, D, S;                    /* minibatch rows, outputs per row (>= 1, any), draws of the WHOLE prediction (>= 1) */
    int32_t form;
    int32_t draw;                       /* ACCUMULATE: 0-based index of this draw; 0 starts the state (nothing is read from it), S - 1 finishes */
    float noise_var;                    /* tau^2 > 0: the log-likelihood is produced; 0: skipped */
    float* state;                       /* ACCUMULATE: R x (2 D + 2) floats, row r = { mean[D], M2[D], sum_s e_s, L } */
    /* outputs of the finish, each optional (NULL to skip) */
    float* mean; float* var; int64_t ld_out;   /* R x D each */
    float* row_var;                     /* R: mean over d of var */
    float* row_sq_err;                  /* R: sum_d (t - mean)^2 (needs target) */
    float* row_log_lik;                 /* R (needs target and noise_var > 0) */
    /* with target: 4 doubles WRITTEN by the finish, { sum_r row_sq_err, sum_{r,s} e_s, sum_r row_log_lik (0 when noise_var is 0),
     * sum_{r,d} var }, each summed over rows in double in a fixed order (workgroup partials, one finish block; no float
     * atomics). NULL to skip. */
    double* totals;
} vbnn_moments_args;
int vbnn_predict_moments(vbnn_ctx* ctx, const vbnn_moments_args* a);

/* The heteroscedastic regression predictive (additive, ABI 6): vbnn_predict_moments for the Gaussian likelihood head of
 * vbnn_gauss_nll_forward. A draw's row holds 2 D floats: columns [0, D) the mean m, columns [D, 2 D) s, the log of the noise
 * variance. Everything stated for vbnn_predict_moments holds here -- fp32 op by op, the row-to-thread assignment, the butterfly
 * and wave-order row sums (their order depends on D alone), the two forms bitwise equal, NaN containment -- with the element
 * and row operations below. Each half of a row (m at column 0, s at column D) takes the 16-byte or the scalar access path on
 * its own alignment. Per element (r, d) and draw, with s_c = min(max(s, s_min), s_max) (a NaN s stays NaN):
 *   Welford on m, exactly as above:  delta = m - mean;  mean = mean + delta / float(s + 1);  M2 = M2 + delta * (m - mean)
 *   v = expf(s_c);   V = v on draw 0, V = V + v on every later draw
 *   with a target:  w = expf(-s_c);  d = t - m;  the element's term of q_s is  s_c + (d * d) * w
 * Per row and draw, with a target: q_s = sum_d (s_c + (d * d) * w);  nll_s = 0.5f * q_s (the draw's negative log density without
 * its constant); sum_s nll_s is kept as a running sum (draw 0 starts it); a_s = -nll_s goes into the online logsumexp: draw 0
 * sets L = a_0, every later draw L = max(L, a) + log1p(exp(-|L - a|)).
 * Finish per element: mean as it stands;  var = M2 / float(S) (the epistemic part);  noise_var = V / float(S) (the aleatoric
 * part; the total predictive variance of an output is var + noise_var).
 * Finish per row: row_var = (sum_d var) / float(D);  row_noise_var = (sum_d noise_var) / float(D);
 *   row_sq_err = sum_d (t - mean)^2;  row_log_lik = L - log(float(S)) - (0.5f * float(D)) * log(6.2831855f)
 * -- the log density of the equal-weight mixture of N(m_s, diag v_s) at the target. */
#define VBNN_GAUSS_MOMENTS_STACKED_MAX_D 8192   /* largest D the STACKED form takes */
typedef struct vbnn_gauss_moments_args {
    const float* y; int64_t ld_y;       /* f32 outputs of the final Linear: S R x 2 D (STACKED) or R x 2 D (ACCUMULATE); ld_y >= 2 D */
    const float* target; int64_t ld_t;  /* R x D regression targets, or NULL */
    int64_t R, D, S;                    /* minibatch rows, outputs per row (the final Linear is 2 D wide), draws of the WHOLE prediction */
    int32_t form;                       /* VBNN_MOMENTS_STACKED or VBNN_MOMENTS_ACCUMULATE */
    int32_t draw;                       /* ACCUMULATE: as in vbnn_moments_args */
    float s_min, s_max;                 /* the clamp of s (s_min <= s_max) */
    float* state;                       /* ACCUMULATE: R x (3 D + 2) floats, row r = { mean[D], M2[D], V[D], sum_s nll_s, L } */
    /* outputs of the finish, each optional (NULL to skip) */
    float* mean; float* var; float* noise_var; int64_t ld_out;   /* R x D each */
    float* row_var;                     /* R: mean over d of var */
    float* row_noise_var;               /* R: mean over d of noise_var */
    float* row_sq_err;                  /* R: sum_d (t - mean)^2 (needs target) */
    float* row_log_lik;                 /* R (needs target) */
    /* with target: 5 doubles WRITTEN by the finish, { sum_r row_sq_err, sum_{r,s} nll_s, sum_r row_log_lik, sum_{r,d} var,
     * sum_{r,d} noise_var }, each summed over rows in double in a fixed order, as vbnn_moments_args.totals. NULL to skip. */
    double* totals;
} vbnn_gauss_moments_args;
int vbnn_predict_gauss_moments(vbnn_ctx* ctx, const vbnn_gauss_moments_args* a);

/* The class-probability posterior predictive for ANY class count (additive, ABI 6): what vbnn_head_predict states above for
 * C <= 16, from the final Linear's f32 logits y_s (R x C per draw, as vbnn_forward writes them) instead of from h, with the
 * top-K classes of the averaged prediction. The third member of the moments family: all arithmetic is fp32, operation by
 * operation as written here (compiled without floating-point contraction; the division is correctly rounded).
 * Per row and draw, in draw order:
 *   mx = max_c y[c], arg_s = its first index;   lse = mx + logf(sum_c expf(y[c] - mx));   o[c] = y[c] - lse
 *   per class the online logsumexp L[c]: draw 0 sets L = o, every later draw L = max(L, o) + log1p(exp(-|L - o|)) -- never a
 *     sum of probabilities, which underflow. Here log1p(u), u = expf(-|L - o|) in [0, 1], is evaluated as
 *     w = 1 + u;  log1p(u) = (logf(w) * u) / (w - 1)  (u itself where w = 1): w - 1 is exact and the correctly rounded quotient
 *     restores what rounding 1 + u lost -- within 3 ulp of log1p, at a fraction of the library log1pf's instructions;
 *   per row the running sums  sum_s H_s with H_s = -sum_c expf(o[c]) * o[c]  and, with a target t (clamped to [0, C - 1]),
 *     sum_s -o[t]  and  sum_s [arg_s = t]  (draw 0 starts each).
 * Finish per row:  log_p[c] = L[c] - logf(float(S));  p[c] = expf(log_p[c]);  entropy = -sum_c p[c] * log_p[c];
 *   expected_entropy = (sum_s H_s) / float(S);  mutual_info = entropy - expected_entropy (S = 1 gives exactly 0);
 *   top-K: K rounds of "the first maximum of log_p among the classes not yet taken" (ties go to the lower index) give
 *   topk_idx (R x K) and topk_prob = expf of that log_p (bitwise probs at topk_idx);  pred = argmax log_p (first maximum),
 *   which is topk_idx[:, 0] when K >= 1.
 * Every row sum (sum_c expf, H_s, entropy) is formed in an order that depends on C alone, by the family's rule: a row is
 * worked by T = 64 threads (C <= 256, four rows per workgroup) or T = 256 (above); thread i adds, in ascending order, the
 * columns 4 q .. 4 q + 3 of its quads q = i, i + T, ...; the threads of a wave are added by the xor butterfly 32, 16, .. 1; the
 * four waves in wave order. Maximum and arg-max reductions take the lower index among equal maxima. The same assignment holds
 * on the 16-byte and on the scalar access path (chosen per launch from the leading dimensions and the base addresses; a row's
 * last, partial quad always goes element by element), in both forms, for every R and row position. Pad columns are never read.
 * Logits are finite or NaN. A NaN logit makes every float output of its row NaN (topk_prob included) and the float totals
 * ([0] and [2]) NaN, and leaves every other row bit for bit alone; pred and topk_idx of such a row are unspecified but inside
 * [0, C - 1]. Infinite logits (-inf as a mask included) are NOT supported in this version: the outputs of such a row are
 * unspecified.
 * VBNN_MOMENTS_STACKED: y holds all S draws (draw s = rows [s R, (s+1) R)); one call walks them with L in registers
 * (C <= VBNN_CLASS_MOMENTS_STACKED_MAX_C; draw / state ignored). VBNN_MOMENTS_ACCUMULATE: y holds ONE draw, number `draw`; the
 * running values live in `state` between the S calls, any C. Both forms run one device function per draw: given the same y per
 * draw, every output and total is bitwise equal between them. */
#define VBNN_CLASS_MOMENTS_STACKED_MAX_C 4096   /* largest C the STACKED form takes */
#define VBNN_CLASS_MOMENTS_MAX_K 8              /* largest K */
typedef struct vbnn_class_moments_args {
    const float* y; int64_t ld_y;       /* f32 logits: S R x C (STACKED; draw s = rows [s R, (s+1) R)) or R x C (ACCUMULATE); ld_y >= C */
    const int32_t* target;              /* R class indices, or NULL: no totals */
    int64_t R, C, S;                    /* minibatch rows, classes (>= 1, any), draws of the WHOLE prediction (>= 1) */
    int32_t form;                       /* VBNN_MOMENTS_STACKED or VBNN_MOMENTS_ACCUMULATE */
    int32_t draw;                       /* ACCUMULATE: 0-based index of this draw; 0 starts the state (nothing is read from it), S - 1 finishes */
    int64_t K;                          /* top-K classes: 0 .. min(VBNN_CLASS_MOMENTS_MAX_K, C) */
    float* state; int64_t ld_state;     /* ACCUMULATE: R x ld_state floats, ld_state >= C + 3, row r = { L[0 .. C-1], sum H, sum -o[t], hits }
                                         * (a multiple of 4 on a 16-byte base takes the 16-byte path) */
    /* outputs of the finish, each optional (NULL to skip -- probs and log_probs too: R x C of stores) */
    float* probs; float* log_probs; int64_t ld_out;   /* R x C each */
    float* entropy;                     /* R: H[p] (total predictive uncertainty) */
    float* expected_entropy;            /* R: 1/S sum_s H(p_s) (the aleatoric part) */
    float* mutual_info;                 /* R: entropy - expected_entropy (the epistemic part) */
    int32_t* pred;                      /* R: argmax p */
    int32_t* topk_idx; float* topk_prob;   /* R x K each (need K >= 1) */
    /* with target: 5 doubles WRITTEN by the finish, { sum_r -log_p[t_r], sum_r [pred = t_r], sum_{r,s} -o_s[t_r],
     * sum_{r,s} [arg_s = t_r], sum_r [t_r in top-K] (0 when K = 0) }, each summed over rows in double in a fixed order (workgroup
     * partials, one finish block; no float atomics). NULL to skip. */
    double* totals;
} vbnn_class_moments_args;
int vbnn_predict_class_moments(vbnn_ctx* ctx, const vbnn_class_moments_args* a);

/* The multi-label posterior predictive (additive, ABI 6): the moments over S draws of the Bernoulli head of vbnn_bce_forward,
 * from the final Linear's f32 logits y_s (R x D per draw). The sixth member of the moments family. Everything stated for
 * vbnn_predict_moments holds here -- fp32 op by op as written (no contraction; correctly rounded divisions; expf / logf /
 * log1pf the library functions), the row-to-thread assignment (T = 64 threads for D <= 256 with four rows per workgroup,
 * T = 256 above; thread i owns the quads q = i, i + T, ...), the xor butterfly and then the waves in wave order, so that every
 * row sum's order depends on D alone, the 16-byte and the scalar access path chosen per launch, pad columns never read, the
 * two forms bitwise equal -- with the element and row operations below.
 * Per element (r, d) and draw, with zc = min(max(z, -80), 80) (a NaN z stays NaN). The clamp floors every probability at
 * e^-80 (a normal fp32), so the sums P and Q below are strictly positive and no log of an average is ever -inf:
 *   u = expf(-|zc|);   w = 1 + u;   l1p = (logf(w) * u) / (w - 1)  (u itself where w == 1)
 *   p = zc >= 0 ? 1 / w : u / w;    q = zc >= 0 ? u / w : 1 / w          -- sigmoid(z) and 1 - sigmoid(z), each on its own
 *   lp = fminf(zc, 0) - l1p;        ln = fminf(-zc, 0) - l1p             -- log p and log q
 *   P = P + p;   Q = Q + q;   Hs = Hs + -(p * lp + q * ln)               (draw 0 sets each)
 *   with a target t:  the element's term of a_s is  t * lp + (1 - t) * ln.
 * Per row and draw, with a target: a_s = sum_d of the element terms (the draw's log-likelihood of the whole label vector); the
 * running sum of -a_s is kept (draw 0 starts it; divided by R S D it is test()'s number for the same draws); a_s goes into the
 * online logsumexp: draw 0 sets L = a_0, every later draw L = max(L, a) + log1pf(expf(-|L - a|)).
 * Finish per element:  pm = P / float(S);  qm = Q / float(S);  log_p = logf(pm);  log_q = logf(qm);
 *   probs = pm;  entropy = -(pm * log_p + qm * log_q);  expected_entropy = Hs / float(S);
 *   mutual_info = entropy - expected_entropy (the per-label BALD score), stored as +0 when S = 1, by definition;
 *   the label is predicted 1 iff P > Q (a tie predicts 0); with a target it is a hit iff that equals (t > 0.5f).
 * Finish per row:  row_entropy = sum_d entropy;  row_mutual_info = sum_d mutual_info;  with a target
 *   row_log_lik = L - logf(float(S))                            -- the JOINT mixture over draws of the whole label vector;
 *   row_marg_log_lik = sum_d (t * log_p + (1 - t) * log_q)      -- the product of the per-label marginals;
 *   row_hits = the number of hits among the D labels (counted in fp32: exact, D < 2^24).
 * A NaN logit makes P, Q, Hs and every float output of its element NaN, the float row values of its row NaN and the float
 * totals NaN; its label counts as a miss; every other element of the row and every other row keep their bits.
 * VBNN_MOMENTS_STACKED: y holds all S draws (draw s = rows [s R, (s+1) R)); one call walks them with P, Q, Hs in registers
 * (D <= VBNN_LABEL_MOMENTS_STACKED_MAX_D; draw / state ignored). VBNN_MOMENTS_ACCUMULATE: y holds ONE draw, number `draw`; the
 * running values live in `state` between the S calls, any D. Both forms run one device function per draw. */
#define VBNN_LABEL_MOMENTS_STACKED_MAX_D 4096   /* largest D the STACKED form takes */
typedef struct vbnn_label_moments_args {
    const float* y; int64_t ld_y;       /* f32 logits: S R x D (STACKED; draw s = rows [s R, (s+1) R)) or R x D (ACCUMULATE); ld_y >= D */
    const float* target; int64_t ld_t;  /* R x D labels in [0, 1], or NULL */
    int64_t R, D, S;                    /* minibatch rows, labels per row (>= 1, any), draws of the WHOLE prediction (>= 1) */
    int32_t form;                       /* VBNN_MOMENTS_STACKED or VBNN_MOMENTS_ACCUMULATE */
    int32_t draw;                       /* ACCUMULATE: 0-based index of this draw; 0 starts the state (nothing is read from it), S - 1 finishes */
    float* state;                       /* ACCUMULATE: R x (3 D + 2) floats, row r = { P[D], Q[D], Hs[D], sum_s -a_s, L } */
    /* outputs of the finish, each optional (NULL to skip) */
    float* probs; float* entropy; float* mutual_info; int64_t ld_out;   /* R x D each */
    float* row_entropy;                 /* R: sum_d entropy */
    float* row_mutual_info;             /* R: sum_d mutual_info */
    float* row_log_lik;                 /* R (needs target) */
    float* row_marg_log_lik;            /* R (needs target) */
    int32_t* row_hits;                  /* R (needs target) */
    /* with target: 5 doubles WRITTEN by the finish, { sum_r row_log_lik, sum_r row_marg_log_lik, sum_{r,s} -a_s, sum_r row_hits,
     * sum_r [row_hits = D] }, each summed over rows in double in a fixed order (workgroup partials, one finish block; no float
     * atomics). NULL to skip. */
    double* totals;
} vbnn_label_moments_args;
int vbnn_predict_label_moments(vbnn_ctx* ctx, const vbnn_label_moments_args* a);

/* Regression predictive quantiles (additive, ABI 6): the fourth member of the moments family. Per element (r, d) the
 * predictive is the equal-weight mixture of S components, one per draw of the final Linear's f32 outputs; this call gives its
 * quantiles at Q probabilities and, with targets, the probability integral transform (PIT) F(t) and the calibration counts
 * #{t <= q_j}. Draw s of row r starts at y + s draw_stride + r ld_y (draw_stride >= R ld_y): a stacked chunk buffer
 * (draw_stride = R ld_y) and a row range of an S x R_total x W draws tensor (draw_stride = R_total W) are both read in place.
 * Draws and targets are finite or NaN. One launch, any D >= 1 and R >= 1 (R < 2^31, every row or plane pitch times its count below 2^60), 1 <= S <= VBNN_QUANTILES_MAX_S, 1 <= Q <=
 * VBNN_QUANTILES_MAX_Q; p strictly ascending, each in [0.001, 0.999]. The file is compiled without floating-point contraction.
 * VBNN_QUANT_EMPIRICAL (a row is D wide; the draws are the distribution): fp32, operation by operation. With a_0 <= .. <=
 * a_{S-1} the element's draws in ascending order (the sign of a zero among equal zeros is unspecified):
 *   pos = p * float(S - 1);  k = min(int(pos), S - 2);  frac = pos - float(k);  q = min(a_k + frac * (a_{k+1} - a_k), a_{k+1})
 *   (S = 1: q = a_0) -- numpy's method "linear"; the final min is part of the contract: where the rounding of the product and
 *   the sum would lift q above a_{k+1} it returns a_{k+1}, which keeps q_j ascending;
 *   pit = float(#{s : y_s <= t}) / float(S) (correctly rounded).
 * VBNN_QUANT_FIXED_NOISE (a row is D wide; component s is N(y_s, noise_var), noise_var > 0) and VBNN_QUANT_GAUSS (a row is
 * 2 D wide, m at column 0 and s at column D; component s is N(m_s, exp(s_c)), s_c = min(max(s, s_min), s_max), the rule of
 * vbnn_predict_gauss_moments): q is the root of F(q) = 1/S sum_s Phi((q - mu_s) / sigma_s) = p. These two kinds are defined by
 * accuracy, not by operation order: the kernel evaluates F in fp32 (a running sum over s of erfcf terms) and returns the
 * upper of two ADJACENT floats lo < q with F32(lo) < p <= F32(q), found by a safeguarded Newton iteration inside a bracket
 * followed by bisection on the floats' ordered bit patterns -- at most 24 + 33 evaluations of F per quantile, a bound that
 * does not depend on the data, and an element's result depends on its own draws alone. So, with eps_F the error allowed to
 * the fp32 evaluation of F:  F(q - 2 ulp) - eps_F <= p <= F(q + 2 ulp) + eps_F  for the exact F -- the exact root of an F
 * perturbed by at most eps_F lies within 2 fp32 ulps of q -- and pit = F(t) within eps_F. (tests/test_quantiles_ref.py
 * measures eps_F; it grows like sqrt(S) 2^-25.) Components are expected to keep sigma_s >= 32 ulp(|mu_s|).
 * Every kind: q_0 <= q_1 <= .. per element. A NaN in any draw of an element (for GAUSS: in m or in s) makes that element's q
 * and pit NaN and no other element's; a NaN target gives a NaN pit; neither counts anywhere. Pad columns and the gaps between
 * draws are never read; for GAUSS the m and s halves never read each other's columns. The draws take 16-byte loads where D,
 * ld_y, draw_stride are multiples of 4 and the half's base address is 16-byte aligned, 4-byte loads otherwise (chosen per
 * launch); outputs and targets go element by element, consecutive threads to consecutive columns. */
enum { VBNN_QUANT_EMPIRICAL = 0, VBNN_QUANT_FIXED_NOISE = 1, VBNN_QUANT_GAUSS = 2 };
#define VBNN_QUANTILES_MAX_S 128   /* most draws */
#define VBNN_QUANTILES_MAX_Q 8     /* most probabilities */
typedef struct vbnn_quantiles_args {
    const float* y; int64_t ld_y;       /* f32 outputs of the final Linear, all S draws; ld_y >= D (GAUSS: >= 2 D) */
    int64_t draw_stride;                /* floats between draw s and draw s + 1 of the same row (>= R ld_y) */
    const float* target; int64_t ld_t;  /* R x D regression targets, or NULL */
    int64_t R, D, S;                    /* rows, outputs per row, draws */
    int32_t kind;                       /* VBNN_QUANT_* */
    int32_t Q;                          /* probabilities in p */
    float p[8];                         /* VBNN_QUANTILES_MAX_Q entries; the first Q are read */
    float noise_var;                    /* FIXED_NOISE: tau^2 > 0 */
    float s_min, s_max;                 /* GAUSS: the clamp of s (s_min <= s_max) */
    /* outputs, each optional (NULL to skip) */
    float* q; int64_t ld_q; int64_t plane_stride;   /* Q planes of R x D: q_j of (r, d) at q + j plane_stride + r ld_q + d */
    float* pit; int64_t ld_pit;         /* R x D (needs target) */
    int32_t* row_le;                    /* R x Q, WRITTEN: entry (r, j) = #{d : t <= q_j} (needs target) */
    uint64_t* count_le;                 /* Q: the call ADDS #{(r, d) : t <= q_j} with integer atomics -- the caller zeroes it; the
                                         * result does not depend on the order, and a chunked call needs no host sum (needs target) */
} vbnn_quantiles_args;
int vbnn_predict_quantiles(vbnn_ctx* ctx, const vbnn_quantiles_args* a);

/* Classifier calibration (additive, ABI 6; vbnn_amd/csrc/calibration.hip): the fifth member of the moments family. From the
 * class probabilities of a predictive (R x C fp32, as vbnn_head_predict / vbnn_predict_class_moments write them), its predicted
 * classes and the targets: per row the confidence, the hit, the Brier score and the confidence bin, and -- added to ONE integer
 * accumulator -- what the reliability diagram, ECE, MCE, the Brier score and the accuracy of a whole test set are computed from.
 * All arithmetic is fp32, operation by operation as written here (compiled without floating-point contraction). Per row r:
 *   p = min(max(pred[r], 0), C - 1);  t = min(max(target[r], 0), C - 1)   (the family's rule for targets)
 *   conf = probs[r, p];   hit = [p == t]
 *   ss = sum_c probs[r, c] * probs[r, c]   by the family's row-sum rule (vbnn_predict_class_moments above: T = 64 threads while
 *     C <= 256, 256 above; thread i adds to +0, in ascending order, the columns 4 q .. 4 q + 3 of its quads q = i, i + T, ...; the
 *     xor butterfly 32, 16, .. 1 inside a wave; the four waves in wave order) -- its order depends on C alone
 *   brier = max((ss - 2 * probs[r, t]) + 1, 0)       (sum_c (probs[c] - [c == t])^2, expanded)
 *   bin = min(int(conf * float(M)), M - 1), M = bins   (evaluated as int(min(max(conf * float(M), 0), float(M - 1))), which is the
 *     same number for every conf >= 0 and keeps any other value inside the M bins)
 * A row whose conf or ss is NaN is SKIPPED: it adds 1 to n_nan and nothing else, its row outputs are NaN (conf, brier) and -1
 * (hit, bin), and no other row changes by a bit. Probabilities are finite values in [0, 1] (a few ulps above 1 included) or NaN;
 * the results for other values are unspecified (no access leaves the buffers). Pad columns (ld > C) are never read; the row
 * takes 16-byte loads where ld is a multiple of 4 and probs is 16-byte aligned, 4-byte loads otherwise (chosen per launch; a
 * row's last, partial quad always goes element by element) -- the same bits either way.
 * acc: 3 M + 4 uint64 words that the call ADDS to and the caller zeroes:
 *   [0, M) count[b];  [M, 2 M) hits[b];  [2 M, 3 M) conf_fix[b] += (uint64)(max(conf, 0) * 2^32)  (the product is exact in fp32; the
 *   conversion truncates nothing once conf >= 2^-9);  [3 M] brier_fix += (uint64)(brier * 2^32);  [3 M + 1] n_rows (the rows
 *   counted: not the NaN ones);  [3 M + 2] n_nan;  [3 M + 3] reserved (untouched).
 * Every accumulated value is an integer, so acc is bit for bit independent of the grid, the arrival order, the chunking, the
 * number of calls and -- summed on the host -- the number of ranks. Each workgroup reduces its rows in LDS first and issues at
 * most one global add per word (64-bit vector integer atomics). From the integers, in float64 on the host:
 *   ECE = sum_b |hits[b] - conf_fix[b] / 2^32| / n_rows;  MCE = max_b |hits[b] - conf_fix[b] / 2^32| / count[b];
 *   Brier = brier_fix / 2^32 / n_rows;  accuracy = sum_b hits[b] / n_rows. */
#define VBNN_CALIBRATION_MAX_BINS 64   /* most bins */
typedef struct vbnn_calibration_args {
    const float* probs; int64_t ld;     /* R x C class probabilities, ld >= C */
    const int32_t* pred;                /* R predicted classes */
    const int32_t* target;              /* R class indices (required) */
    int64_t R, C;                       /* rows (1 .. 2^31 - 1), classes (>= 1) */
    int32_t bins;                       /* M: 1 .. VBNN_CALIBRATION_MAX_BINS equal-width confidence bins */
    int32_t reserved;
    /* per-row outputs, each optional (NULL to skip) */
    float* conf; int32_t* hit; float* brier; int32_t* bin;   /* R each */
    uint64_t* acc;                      /* 3 bins + 4 words: the call ADDS, the caller zeroes (8-byte aligned) */
} vbnn_calibration_args;
int vbnn_predict_calibration(vbnn_ctx* ctx, const vbnn_calibration_args* a);

/* Selective prediction (same file): the risk against the coverage at chosen ranks. score (R fp32, lower = more certain: an
 * entropy, a mutual information, 1 - conf) orders the rows, hit (R int32, nonzero = correct) says which were right. Scores order
 * as floats by their bits: with u the bits of a score, key = u ^ (u >> 31 ? 0xffffffff : 0x80000000), compared as unsigned
 * integers -- -0 sorts right below +0, -inf first; every NaN counts as the positive quiet NaN 0x7fc00000, above +inf (rows
 * with a NaN score rank last). For each of the Q ranks k[j] (1-based, 1 <= k <= R; any order, repeats allowed):
 *   tau[j] = the score of the k[j]-th smallest key (the quiet NaN when that is a NaN);
 *   counts[4 j ..] = { n_below, hits_below, n_tied, hits_tied }: the rows whose key is below tau's and the hits among them, the
 *   rows whose key EQUALS tau's and the hits among them (n_below < k <= n_below + n_tied).
 * Ties are NOT broken by row order: the accuracy at rank k is the expectation over a random tie-break,
 *   acc@k = (hits_below + (k - n_below) * hits_tied / n_tied) / k   (float64, on the host),
 * so scores that are all equal (the mutual information of a MAP or one-draw prediction is exactly 0 on every row) give the
 * overall accuracy at every k, not the accuracy of the first k rows. An exact radix select on integer counts in one workgroup
 * (R is a test set; R < 2^31): no float atomics, no allocation, no host synchronisation; tau and counts are WRITTEN. */
#define VBNN_SELECTIVE_MAX_Q 32        /* most ranks */
typedef struct vbnn_selective_args {
    const float* score;                 /* R */
    const int32_t* hit;                 /* R */
    int64_t R;
    int32_t Q;                          /* ranks in k */
    int32_t reserved;
    int64_t k[32];                      /* VBNN_SELECTIVE_MAX_Q entries; the first Q are read */
    float* tau;                         /* Q */
    uint64_t* counts;                   /* Q x 4 (8-byte aligned) */
} vbnn_selective_args;
int vbnn_selective(vbnn_ctx* ctx, const vbnn_selective_args* a);

/* Conformal prediction sets (additive, ABI 6; vbnn_amd/csrc/conformal.hip; not in the reference): split conformal prediction
 * for a class predictive. From the class probabilities (R x C fp32) the call computes a per-row conformity score of the target
 * and, for Q thresholds, the set of classes whose score is at or below the threshold. A threshold is one exact order statistic
 * of the scores of a held-out calibration set (vbnn_selective on `score` gives it); the sets then hold the true class with at
 * least the requested probability for exchangeable data, whatever the network. All arithmetic is fp32, operation by operation
 * as written here (compiled without floating-point contraction).
 * RANKING of a row. With w(x) = the order word of x's bits (vbnn_selective's map: sign clear -> b ^ 0x80000000, sign set -> ~b,
 * compared as unsigned integers), class c ranks AT OR ABOVE class j iff w(p[c]) > w(p[j]), or w(p[c]) == w(p[j]) and c <= j:
 * larger probabilities first, ties to the lower index (the project's rule everywhere), -0 below +0.
 * SCORES. t = min(max(target[r], 0), C - 1) (the family's rule for targets).
 *   VBNN_CONFORMAL_LAC: s(r, j) = 1 - p[j].
 *   VBNN_CONFORMAL_APS (adaptive prediction sets, not randomised): s(r, j) = sum_c m_c with m_c = p[c] if c ranks at or above
 *     j (j itself included), else +0 -- a MASKED row sum over all C columns by the family's row-sum rule as
 *     vbnn_predict_calibration states it: T = 64 threads while C <= 256, 256 above; thread i adds to +0, in ascending order,
 *     the columns 4 q .. 4 q + 3 of its quads q = i, i + T, ...; the xor butterfly 32, 16, .. 1 inside a wave; the four waves in
 *     wave order. The order depends on C alone, not on the mask.
 * SETS. set_q(r) = { j : s(r, j) <= qhat[q] }, an fp32 comparison; a NaN qhat[q] is taken as +inf (every class). What the
 * method rests on: ALONG A ROW'S RANKING s IS NON-DECREASING IN FP32, SO THE SET IS A PREFIX OF THE RANKING. (LAC: p does not
 * increase along the ranking and fl(1 - p) is monotone in p. APS: going down the ranking only turns terms of the sum from +0
 * into a p[c] >= 0 at a fixed place of a fixed tree of additions, and a rounded addition is monotone in either argument, so
 * no node of the tree decreases. Equal probabilities have equal LAC scores, and their APS scores follow the index.)
 *   size[q, r] = the prefix length;  cut_index / cut_prob[q, r] = the index and the probability (a copy of its bits) of the
 *   last admitted class, -1 and the quiet NaN 0x7fc00000 for an empty set;  member = the prefix as bits (class j is bit j & 31
 *   of word j >> 5 of the row's ceil(C / 32) words; the unused high bits of the last word are zero);
 *   covered[q, r] = [s(r, t) <= qhat[q]], which is the member bit of t;  score[r] = s(r, t).
 * A row whose UNMASKED row sum (every m_c = p[c], the same rule) is NaN is SKIPPED: it adds 1 to n_nan and nothing else, its
 * score and cut_prob are NaN, its size, cut_index and covered are -1, its member words 0, and no other row changes by a bit.
 * Probabilities are finite values in [0, 1] (a few ulps above 1, -0 and subnormals included) or NaN; the results for other values
 * are unspecified (no access leaves the buffers). Pad columns (ld > C) are never read; the row takes 16-byte loads where ld is a
 * multiple of 4 and probs is 16-byte aligned, 4-byte loads otherwise (chosen per launch; a row's last, partial quad always goes
 * element by element) -- the same bits either way.
 * acc: 8 Q + 2 uint64 words that the call ADDS to and the caller zeroes. Per threshold q, words 8 q + 0 .. 8 q + 7:
 *   0 rows counted (not the NaN ones);  1 covered;  2 sum of size;  3 empty sets;  4 singletons;  5 covered singletons;
 *   6 full sets (size == C);  7 reserved (untouched).   acc[8 Q] = n_nan;  acc[8 Q + 1] reserved (untouched).
 * Words 1 and 5 are untouched without target. Every accumulated value is an integer, so acc is bit for bit independent of the
 * grid, the arrival order, the chunking, the number of calls and -- summed on the host -- the number of ranks. Each workgroup
 * reduces its rows in LDS first and issues at most one global add per word (64-bit vector integer atomics). From the integers,
 * in float64 on the host: coverage = covered / rows, mean size = sum of size / rows, and the fractions likewise.
 * Refused with VBNN_ERR_INVALID and nothing written: an unknown kind; Q outside [0, VBNN_CONFORMAL_MAX_Q]; qhat NULL with Q > 0
 * (it is not read with Q = 0); score or covered without target; R or C out of range; ld < C; a pointer that is not 4-byte aligned
 * (acc: 8). The thresholds are read on the device: no host synchronisation, no allocation. */
#define VBNN_CONFORMAL_MAX_Q 8         /* most thresholds */
#define VBNN_CONFORMAL_LAC 0
#define VBNN_CONFORMAL_APS 1
typedef struct vbnn_conformal_args {
    const float* probs; int64_t ld;     /* R x C class probabilities, ld >= C */
    const int32_t* target;              /* R class indices, or NULL */
    int64_t R, C;                       /* rows (1 .. 2^31 - 1), classes (>= 1) */
    int32_t kind;                       /* VBNN_CONFORMAL_LAC | VBNN_CONFORMAL_APS */
    int32_t Q;                          /* thresholds: 0 (scores only) .. VBNN_CONFORMAL_MAX_Q */
    const float* qhat;                  /* Q thresholds ON THE DEVICE; NULL iff Q = 0 */
    /* outputs, each optional (NULL to skip) */
    float* score;                       /* R: s(r, t_r) (needs target) */
    int32_t* size;                      /* Q x R */
    int32_t* cut_index;                 /* Q x R */
    float* cut_prob;                    /* Q x R */
    int32_t* covered;                   /* Q x R (needs target) */
    uint32_t* member;                   /* Q x R x ceil(C / 32) words */
    uint64_t* acc;                      /* 8 Q + 2 words: the call ADDS, the caller zeroes (8-byte aligned) */
} vbnn_conformal_args;
int vbnn_conformal(vbnn_ctx* ctx, const vbnn_conformal_args* a);

/* Conformal intervals for a regression predictive (additive, ABI 6; vbnn_amd/csrc/conformal_interval.hip; not in the reference):
 * split conformal prediction with one order statistic per output. Three scores are ONE expression on different planes. With a
 * lower plane a, an upper plane b (R x D fp32, row pitch ld; plane pair p at + p * plane_stride, plane_stride = 0 when all levels
 * share one pair), an optional width w and a target t, all fp32, one rounding per operation as written (no fused multiply-add;
 * the division and the square root correctly rounded):
 *   v = scale[r, d] (+ scale2[r, d] when scale2 is given), then v = v + scale_add (always added);
 *   u = sqrtf(v) when scale_is_variance, else v;   w = w_min where u < w_min, else u (a NaN u stays NaN; w_min > 0);
 *   m = the larger of (a - t) and (t - b), NaN when either difference is NaN;
 *   s = m / w with a scale plane, m without (no division);
 *   interval at the threshold q:  lo' = a - q * w,  hi' = b + q * w  (the product, then the sum; q itself without a scale);
 *   covered = [ s <= q ], a float comparison; a NaN q is taken as +inf.
 * "absolute": a = b = the mean, no scale (s = |t - mean| exactly). "scaled": a = b = the mean, scale = the variance(s).
 * "cqr" (conformalised quantile regression): a, b the lower and upper quantile planes of every level, no scale; q may be
 * negative, lo' > hi' is an EMPTY interval and is counted. COVERED FOLLOWS THE SCORE, not a comparison of t with the rounded end
 * points: the two differ for targets within a few ulps of an end point, and only the score is the statistic that was calibrated.
 * A NaN ELEMENT of plane pair p: a, b or w is NaN, or -- with a target -- s is NaN (a NaN t; inf - inf). Inputs are finite
 * or NaN; other values give what the operations above give.
 * SCORE MODE, Q = 0 (target required): score[p, r, d] = s (the quiet NaN 0x7fc00000 for a NaN element), row_score[p, r] = the
 * maximum of the row's scores, NaN if any is NaN (a maximum is exact: no order rule). acc: 2 words, ADDED to:
 *   { NaN elements, rows with a NaN element }, both over all P plane pairs.
 * INTERVAL MODE, 1 <= Q <= VBNN_CONFORMAL_MAX_Q, P = 1 or P = Q (level j reads plane pair j). The thresholds are read ON THE
 * DEVICE: level j, column d at qhat[j * ld_qhat + (per_column ? d : 0)]. Outputs, each optional: lo, hi (Q x R x D; the quiet
 * NaN for a NaN element); with a target covered (Q x R x D uint8: 1 / 0, 255 for a NaN element) and row_covered (Q x R int32:
 * the row's covered outputs, -1 for a row with a NaN element). acc: 8 Q + 2 uint64 words, ADDED to. Per level j, 8 j + ..:
 *   0 elements counted (not the NaN ones);  1 covered elements;  2 rows counted (those without a NaN element);
 *   3 rows with EVERY output covered;  4 empty intervals (lo' > hi') among the elements counted;  5 .. 7 reserved (untouched).
 *   acc[8 Q] = NaN elements, acc[8 Q + 1] = rows with a NaN element, both over the P plane pairs.
 * Words 1 and 3 are untouched without a target. A NaN element changes no other element by a bit. Every accumulated value is an
 * integer: acc is bit for bit independent of the grid, the arrival order, the chunking and the number of calls; a workgroup
 * reduces in LDS and issues at most one global add per word. Loads and stores are 16-byte where every pitch in use (ld, ld_s,
 * ld_t, plane_stride; D for the outputs) is a multiple of 4 and the bases are 16-byte aligned, 4-byte otherwise, chosen per
 * launch -- the same bits either way. Pad columns are never read.
 * Refused with VBNN_ERR_INVALID and nothing written: P outside [1, 8]; Q outside [0, 8]; Q >= 1 with P not in {1, Q}; Q = 0
 * without target; covered or row_covered without target; score or row_score with Q >= 1; lo, hi, covered or row_covered with
 * Q = 0; qhat NULL with Q >= 1; scale2 without scale; w_min not above 0 with a scale; R or D out of range; a pitch below D; a
 * pointer that is not 4-byte aligned (acc: 8). No host synchronisation, no allocation. */
typedef struct vbnn_conformal_interval_args {
    const float* lower; const float* upper;   /* P plane pairs of R x D (the same pointer for a = b) */
    int64_t ld;                         /* row pitch of both, >= D */
    int64_t plane_stride;               /* floats between plane pairs; 0: one pair for every level (P = 1) */
    int32_t P;                          /* plane pairs: 1 .. VBNN_CONFORMAL_MAX_Q */
    int32_t Q;                          /* thresholds: 0 (score mode) .. VBNN_CONFORMAL_MAX_Q */
    const float* scale; const float* scale2;  /* R x D each, or NULL (scale2 needs scale) */
    int64_t ld_s;                       /* row pitch of both, >= D */
    float scale_add;                    /* added to the scale sum */
    int32_t scale_is_variance;          /* nonzero: the width is the square root */
    float w_min;                        /* smallest width (> 0) */
    int32_t per_column;                 /* nonzero: a threshold per column */
    const float* target; int64_t ld_t;  /* R x D, or NULL (interval mode only) */
    int64_t R, D;                       /* rows (1 .. 2^31 - 1), outputs (>= 1) */
    const float* qhat; int64_t ld_qhat; /* thresholds ON THE DEVICE; NULL iff Q = 0 */
    /* outputs, each optional (NULL to skip) */
    float* score;                       /* P x R x D (score mode) */
    float* row_score;                   /* P x R (score mode) */
    float* lo; float* hi;               /* Q x R x D */
    uint8_t* covered;                   /* Q x R x D (needs target) */
    int32_t* row_covered;               /* Q x R (needs target) */
    uint64_t* acc;                      /* 2 (score mode) or 8 Q + 2 words: the call ADDS, the caller zeroes (8-byte aligned) */
} vbnn_conformal_interval_args;
int vbnn_conformal_interval(vbnn_ctx* ctx, const vbnn_conformal_interval_args* a);

/* Column-wise order statistics (same file): for every column d of an R x D fp32 matrix x (row pitch ld) and each of Q ranks
 * k[j] (1-based, 1 <= k <= R, shared by the columns; any order, repeats allowed),
 *   tau[j * ld_tau + d] = the value of the k[j]-th smallest key of column d under vbnn_selective's key rule exactly (order word
 *   of the bits, -0 below +0, every NaN the positive quiet NaN 0x7fc00000 above +inf);
 *   counts[(j * D + d) * 2 ..] = { keys below tau's, keys equal to tau's } (optional);  n_nan[d] = NaN keys (optional).
 * All outputs are WRITTEN. An exact radix select on integer counts (four 8-bit digits; a workgroup owns 16 neighbouring
 * columns), bit for bit independent of the grid; no float atomics, no allocation, no host synchronisation. D = 1 is one
 * workgroup, as vbnn_selective is. Refused with VBNN_ERR_INVALID: a null x or tau; R outside [1, 2^31); D < 1; ld < D; ld_tau
 * < D; Q outside [1, VBNN_SELECT_COLUMNS_MAX_Q]; a rank outside [1, R]; a pointer that is not 4-byte aligned. */
#define VBNN_SELECT_COLUMNS_MAX_Q 8    /* most ranks */
typedef struct vbnn_select_columns_args {
    const float* x; int64_t ld;         /* R x D, ld >= D */
    int64_t R, D;
    int32_t Q;                          /* ranks in k */
    int32_t reserved;
    int64_t k[8];                       /* VBNN_SELECT_COLUMNS_MAX_Q entries; the first Q are read */
    float* tau; int64_t ld_tau;         /* Q x D, ld_tau >= D */
    uint32_t* counts;                   /* Q x D x 2, or NULL */
    uint32_t* n_nan;                    /* D, or NULL */
} vbnn_select_columns_args;
int vbnn_select_columns(vbnn_ctx* ctx, const vbnn_select_columns_args* a);

/* ---- pool acquisition for active learning (additive, ABI 6; vbnn_amd/csrc/acquire.hip; not in the reference) ----------------
 * vbnn_top_rows: the exact top-k of R fp32 scores WITH their row indices -- which rows of an unlabelled pool to label next.
 * ORDER. A key orders by its bits under vbnn_selective's monotone map (sign clear -> b ^ 0x80000000, sign set -> ~b, compared
 * as unsigned integers): -0 ranks below +0, +-inf are ordinary values. A row whose SCORE is a NaN (any pattern) is never a
 * candidate and is counted in n_nan; a row with exclude[r] != 0 is never a candidate and is counted in n_excluded ONLY (its score
 * is not looked at). Among equal keys the LOWER row index wins and comes first. The output is fully ordered -- by key (largest = 1:
 * descending, largest = 0: ascending), then by ascending row index -- and is bit for bit the same whatever the grid and the
 * order in which the atomics arrive. With fewer than k candidates n_selected is their number; the remaining index entries are -1
 * and their value / key entries the quiet NaN 0x7fc00000.
 * KEY. stochastic = 0: key = score. stochastic = 1 (sampling k rows without replacement with probability proportional to
 * score^beta: Gumbel top-k in its exponential-race form), evaluated op for op from vbnn_philox.h, for global row g = row0 + r:
 *   x   = word (g & 3) of vbnn_philox4x32_10(g >> 2, 0, draw, VBNN_STREAM_ACQUIRE, (uint32_t)seed, (uint32_t)(seed >> 32))
 *   u   = (float)min((x >> 8) + 1, 2^24 - 1) * 2^-24                       (0 < u < 1, exact)
 *   E   = -vbnn_det_logf(u)                                                (> 0: a unit exponential)
 *   L   = vbnn_det_logf(s) for a positive normal finite score s;  +inf for s = +inf;  -inf for every other non-NaN s (zero,
 *         negative, subnormal: still candidates, chosen last);  0 when score is NULL (every candidate has weight 1)
 *   key = fmaf(beta, L, -vbnn_det_logf(E))
 * and the top k by key with largest = 1 (largest = 0 is refused). The noise depends on (seed, draw, g) alone: a pool scored in
 * pieces, each with its row0, gets the keys of the whole. vbnn_det_logf is used beyond the [2^-24, 1] its comment states (E up to
 * 16.7, scores over the normal range); the relative error measured there is in DESIGN.md section 8.
 * OUTPUTS, all WRITTEN: index[j] the selected rows; value[j] = score[index[j]] as given (a bit copy; 1.0f when score is NULL);
 * key[j] (optional) the key the row was ranked by (stochastic = 0: the score's bits); counts = { n_selected, n_candidates,
 * n_nan, n_excluded }.
 * SHAPE: three digit passes (11 + 11 + 10 bits, an LDS histogram per workgroup, one integer atomic per non-empty bin) find the
 * k-th key and how many of its tied rows are wanted; a count pass per workgroup (skipped on the device unless the tie must be
 * split) and one take pass collect the rows, ties by a prefix in index order over contiguous row ranges; one workgroup sorts the
 * <= 4096 (key, row) pairs in LDS. stochastic = 0: keys are re-formed in every pass, 4 B (+ 1 B of exclude) read per row and
 * pass, nothing per row written. stochastic = 1: the first pass stores every row's key in the workspace (4 B per row) and the
 * later passes read it. A 16-byte aligned score (with exclude NULL or 4-byte aligned) takes 16-byte loads, any other 4-byte
 * aligned score the 4-byte path; the stored keys likewise by the workspace's alignment. Integer atomics only, no allocation, no
 * host synchronisation; the workspace (a fixed part and 4 B per row; vbnn_top_rows_workspace_bytes) needs no preparation.
 * VBNN_ERR_INVALID, nothing written: R outside 1 .. 2^31 - 1; k outside 1 .. VBNN_TOP_ROWS_MAX_K; score NULL with
 * stochastic = 0; largest = 0 with stochastic = 1; beta not in (0, FLT_MAX]; row0 < 0 or row0 + R > 2^32; a NULL output or
 * workspace; workspace_bytes below vbnn_top_rows_workspace_bytes; a misaligned pointer (4 bytes; counts 8). */
#define VBNN_TOP_ROWS_MAX_K 4096       /* most rows selected in one call */
typedef struct vbnn_top_rows_args {
    const float*   score;               /* R, or NULL with stochastic = 1: every candidate has weight 1 ("random") */
    const uint8_t* exclude;             /* R or NULL; non-zero = not a candidate */
    int64_t R;                          /* 1 <= R < 2^31 */
    int32_t k;                          /* 1 .. VBNN_TOP_ROWS_MAX_K */
    int32_t largest;                    /* 1: the k largest keys; 0: the k smallest */
    int32_t stochastic;                 /* 0: key = score; 1: the perturbed key above */
    float   beta;                       /* stochastic: > 0, finite */
    uint64_t seed; uint32_t draw; int64_t row0;   /* stochastic: noise address; row0 + R <= 2^32 */
    int32_t* index;                     /* k: selected rows, ordered by (key, then LOWER index first) */
    float*   value;                     /* k: score[index[j]] as given (bit copies) */
    float*   key;                       /* k or NULL: the key each row was ranked by */
    int64_t* counts;                    /* 4: n_selected, n_candidates, n_nan, n_excluded (WRITTEN) */
    void* workspace; size_t workspace_bytes;
} vbnn_top_rows_args;
int vbnn_top_rows_workspace_bytes(int64_t R, int32_t k, size_t* bytes);
int vbnn_top_rows(vbnn_ctx* ctx, const vbnn_top_rows_args* a);

/* ---- diverse pool acquisition: greedy k-centre selection (additive, ABI 6; vbnn_amd/csrc/kcentre.hip; not in the reference) --
 * vbnn_kcentre: core-set selection (Sener & Savarese) over R rows of D fp32 features. Each of k steps takes the candidate
 * farthest from every centre so far -- the given `centres` and the rows picked before it -- optionally weighted by a per-row
 * score. All arithmetic is fp32, operation by operation as written here (compiled without floating-point contraction: no
 * multiply-add is fused); the output is bit for bit the same whatever the grid and the order in which the atomics arrive.
 * DISTANCE. d(r, c) = sum_j (f[r,j] - f[c,j])^2. The row is shared by T threads, T = 64 for D <= 1024 and T = 256 above. With the
 * row cut into quads of four columns (the last one short), thread i owns quads i, i + T, i + 2T, ... and walks its columns in
 * ascending order from acc = +0:  t = f[r,j] - f[c,j];  p = t * t;  acc = acc + p  (three roundings per column). The T partials
 * are added by the moments family's row-sum rule: inside each wave of 64 lanes the xor butterfly v[i] = v[i] + v[i ^ off] for
 * off = 32, 16, 8, 4, 2, 1; for T = 256 the four waves then as ((w0 + w1) + w2) + w3. The order depends on D alone. d(r, r) is
 * exactly +0. The squared NORM of a row is the same sum with f[c,j] = 0 and no subtraction (p = f * f).
 * VOID. A row whose squared norm is not finite (a NaN, an infinity, an overflow) is void: never a candidate, ignored as a
 * centre, counted in n_void, min_dist = the quiet NaN 0x7fc00000. With resume = 1 no norm is taken: a row is void exactly when
 * the min_dist given for it is a NaN (it is rewritten as 0x7fc00000).
 * MINIMUM. m[r] = min over the centres so far of d(r, c) (m = d < m ? d : m), from +inf, or from the given min_dist with
 * resume = 1. The given centres are applied first, in blocks (the result does not depend on the blocks: a minimum). A centre
 * index outside [0, R) is ignored; how many were is left as an int64 in the first 8 bytes of the workspace on return.
 * CANDIDATES are the rows that are not excluded (exclude[r] == 0), not void and not picked in this call. A candidate whose
 * weight is a NaN or below zero (-0 is not) is no candidate either and is counted in n_void, but its min_dist is kept and it
 * serves as a centre when given as one. An excluded row is counted in n_excluded only. n_candidates counts the candidates
 * before the first step. A given centre that is not excluded stays a candidate (with m = 0).
 * KEY of a candidate: m (weight NULL) or m * w (one multiplication) while m is finite; w, or +inf with weight NULL, while
 * m = +inf (no centre yet, or every distance overflowed). The one NaN product, 0 * inf, counts as +0. Each step takes the
 * candidate with the LARGEST key, keys ordered as vbnn_top_rows orders them (the monotone map of their bits, -0 below +0),
 * ties to the LOWER row; it records index[t], key[t] and dist[t] = the pick's m before it was picked; the pick becomes a
 * centre. When the candidates run out n_selected < k, the rest of index is -1 and the rest of key / dist is 0x7fc00000.
 * min_dist on return is m after the last pick (picked rows hold +0). A call with k = a + b gives the bits of a call with
 * k = a followed by one with resume = 1, the a picks added to exclude, and k = b.
 * OUTPUTS, all WRITTEN: index, key, dist (k each), min_dist (R), counts = { n_selected, n_candidates, n_void, n_excluded }.
 * SHAPE: initial centres in blocks of min(8, 32768 / (4 * ceil(D / 4))) rows staged in LDS, one pass over feat per block;
 * then k + 1 launches, each staging the previous pick's row (read from a device word), lowering m, and settling its own pick
 * with one 64-bit integer atomic max of (order word << 32 | ~row) per workgroup; a one-workgroup finish. The first launch also
 * takes the norms and writes one byte per row of workspace (candidate or not). feat with a 16-byte aligned base and ld % 4 == 0
 * takes 16-byte loads, an 8-byte aligned base with ld % 2 == 0 8-byte loads, anything else 4-byte loads; a short last quad
 * is read element by element, so nothing past column D - 1 is read. No allocation, no host synchronisation, no workgroup waits
 * for another; the workspace (vbnn_kcentre_workspace_bytes: a fixed part and 1 B per row) needs no preparation.
 * VBNN_ERR_INVALID, nothing written: R outside 1 .. 2^31 - 1; D outside 1 .. VBNN_KCENTRE_MAX_D; k outside 1 ..
 * VBNN_KCENTRE_MAX_K; ld < D; n_centres < 0, or centres NULL with n_centres > 0; resume not 0 / 1; a NULL feat, index, min_dist,
 * counts or workspace (key and dist are optional); workspace_bytes below vbnn_kcentre_workspace_bytes; a misaligned pointer
 * (4 bytes; counts and the workspace 8). */
#define VBNN_KCENTRE_MAX_K 4096        /* most rows selected in one call */
#define VBNN_KCENTRE_MAX_D 8192        /* widest feature row */
typedef struct vbnn_kcentre_args {
    const float*   feat;                /* R x D, row stride ld */
    int64_t ld;                         /* >= D */
    const float*   weight;              /* R or NULL */
    const uint8_t* exclude;             /* R or NULL; non-zero = never taken */
    const int32_t* centres;             /* n_centres rows already labelled (duplicates, excluded and void rows allowed) or NULL */
    int64_t R;                          /* 1 <= R < 2^31 */
    int64_t D;                          /* 1 .. VBNN_KCENTRE_MAX_D */
    int32_t n_centres;                  /* >= 0 */
    int32_t k;                          /* 1 .. VBNN_KCENTRE_MAX_K */
    int32_t resume;                     /* 1: m starts from min_dist as given */
    int32_t reserved;                   /* 0 */
    int32_t* index;                     /* k: the picks in pick order */
    float*   key;                       /* k or NULL */
    float*   dist;                      /* k or NULL */
    float*   min_dist;                  /* R: read with resume = 1, WRITTEN */
    int64_t* counts;                    /* 4: n_selected, n_candidates, n_void, n_excluded (WRITTEN) */
    void* workspace; size_t workspace_bytes;
} vbnn_kcentre_args;
int vbnn_kcentre_workspace_bytes(int64_t R, int64_t D, int32_t k, size_t* bytes);
int vbnn_kcentre(vbnn_ctx* ctx, const vbnn_kcentre_args* a);

/* ---- rank metrics: exact AUROC and average precision per label (additive, ABI 6; vbnn_amd/csrc/ranking.hip; not in the
 * reference) -- vbnn_rank_metrics: per column j of an R x D fp32 score matrix (row pitch ld >= D; pad columns are never read),
 * the integers that AUROC, average precision and the hit counts at Q thresholds are ratios of.
 * LABELS. Exactly one of two sources: `target` (R x D fp32, pitch ld_t >= D): element (r, j) is positive iff t > 0.5f, the
 * Bernoulli criterion's own hit rule; or `target_class` (R int32): column j is positive on row r iff
 * min(max(t, 0), D - 1) == j, the moments family's target rule, one-vs-rest.
 * COUNTED. An element is counted unless its score is a NaN or, with `target`, its target is a NaN. An element that is not
 * counted adds 1 to n_nan and changes nothing else.
 * ORDER. That of the fp32 values: -0 equals +0 (the score is canonicalised as s + 0.0f -- in the kernel the bit pattern
 * 0x80000000 becomes 0, which is that sum for every non-NaN s without depending on a denormal mode -- before vbnn_selective's
 * monotone map: sign clear -> b ^ 0x80000000, sign set -> ~b, compared as unsigned integers); +-inf are ordinary values;
 * subnormals order as they are. A threshold compares the same way (s >= tau[q] as fp32 values; a NaN tau[q] is met by nothing).
 * OUTPUTS, all WRITTEN (rank metrics are not additive over rows): out holds D x (6 + 2 Q) uint64 words, column j at
 * out + j (6 + 2 Q):
 *   [0] n_pos, [1] n_neg, [2] n_nan;
 *   [3] u2 = sum over the positives i of (2 #{negatives k : s_k < s_i} + #{negatives k : s_k == s_i}); AUROC = u2 / (2 n_pos
 *       n_neg), ties counted half; u2 <= 2^61 for R < 2^31;
 *   [4] ap_fix = sum over the positives i of floor(TP_i 2^32 / (TP_i + FP_i)), TP_i = #{positives : s >= s_i}, FP_i =
 *       #{negatives : s >= s_i}; average precision = ap_fix / (2^32 n_pos): the step-wise sum_n (R_n - R_{n-1}) P_n over the
 *       distinct thresholds. Each term is below its exact value by less than 1, so the host value is within 2^-32 below the
 *       exact rational; TP 2^32 <= 2^63 and ap_fix <= 2^63: no overflow;
 *   [5] reserved (written 0);
 *   [6 + 2 q] tp_q = #{positives : s >= tau[q]}, [7 + 2 q] fp_q = #{negatives : s >= tau[q]} for q < Q (any floats, any order).
 * Everything is an integer: out is bit for bit the same whatever the grid, the order in which the atomics arrive, and the
 * arrangement of the sort.
 * SHAPE. out is cleared; a pack pass (tiles of 4096 elements through LDS; 4 B of score and 4 B of target read with 4-byte
 * loads, whatever the alignment) writes one 8-byte record (order word << 1 | positive; all ones for an element that is not
 * counted, which sorts last) per element, column-major, into the first half of the workspace, and adds n_pos / n_neg / n_nan /
 * tp_q / fp_q -- kept in registers over a workgroup's tiles, then one LDS add per thread and one 64-bit integer atomic per
 * nonzero word and workgroup. Then ONE workgroup of 1024 threads per column: one read for the four 8-bit digit histograms of
 * the order word, a stable least-significant-digit radix pass per digit through the two halves of the workspace (the rank inside
 * a wave from ballots on the digit's bits, the waves' digit counts prefixed in wave order in LDS, tiles in row order; a digit
 * on which the whole column agrees is skipped), and a walk over the sorted column that carries the running positive and
 * negative counts across tiles and closes each run of equal order words with its share of u2 and ap_fix (a 64-bit division per
 * run). Passes over the 8-byte records: 1 written by the pack, 1 read for the histograms, up to 4 read and written by the
 * sort, 1 read by the walk. There is no parallelism inside a column.
 * Integer atomics only, no allocation, no host synchronisation. The workspace needs no preparation;
 * vbnn_rank_metrics_workspace_bytes gives 16 R D bytes (two 8-byte records per element, nothing else).
 * VBNN_ERR_INVALID, nothing written: R < 1, D < 1, R D > 2^31 - 1; Q outside 0 .. VBNN_RANK_MAX_Q; ld < D, or ld_t < D with
 * target; both or neither of target / target_class; a NULL score, out or workspace; workspace_bytes below
 * vbnn_rank_metrics_workspace_bytes; a misaligned pointer (4 bytes; out and the workspace 8). */
#define VBNN_RANK_MAX_Q 16             /* most thresholds */
typedef struct vbnn_rank_metrics_args {
    const float* score; int64_t ld;     /* R x D scores, ld >= D */
    const float* target; int64_t ld_t;  /* R x D fp32 labels (positive iff > 0.5f), ld_t >= D; or NULL */
    const int32_t* target_class;        /* R class indices (one-vs-rest); or NULL */
    int64_t R, D;                       /* rows, columns: R D <= 2^31 - 1 */
    int32_t Q;                          /* thresholds in tau: 0 .. VBNN_RANK_MAX_Q */
    int32_t reserved;
    float tau[16];                      /* VBNN_RANK_MAX_Q entries; the first Q are read */
    uint64_t* out;                      /* D x (6 + 2 Q) words, WRITTEN (8-byte aligned) */
    void* workspace; size_t workspace_bytes;
} vbnn_rank_metrics_args;
int vbnn_rank_metrics_workspace_bytes(int64_t R, int64_t D, size_t* bytes);
int vbnn_rank_metrics(vbnn_ctx* ctx, const vbnn_rank_metrics_args* a);

/* ---- the sampling-free predictive by moment propagation (additive, ABI 6; vbnn_amd/csrc/propagate.hip; not in the reference) --
 * A factorised-Gaussian posterior needs no draws to predict: one pass carries (mean a, second moment q, variance c) of every
 * activation through the network. A hidden layer is three SINGLE products of vbnn_forward (w2 = NULL, y out, no ReLU):
 *   m = a mu^T + b,   v1 = q (sigma^2)^T,   v2 = c (mu^2)^T      (the first layer's input is deterministic: a = x, q = x . x, no v2)
 * -- Var[sum_i w_i h_i] = sum_i (sigma_i^2 E[h_i^2] + mu_i^2 Var[h_i]) for independent w and h, unit correlations dropped -- then
 * vbnn_relu_moments; the final Linear gives the output mean a w3^T + b3 and the output variance c (w3^2)^T. The three calls
 * below are the pieces that are not a GEMM. All three calls' arithmetic is fp32, operation by operation as written here
 * (compiled without floating-point contraction; sqrt and the division are correctly rounded; expf / erfcf are the library
 * functions). Non-finite inputs and negative variances are out of contract: the outputs of such an element are unspecified
 * (no other element is affected).
 *
 * vbnn_relu_moments: per element of an N x O block, the moments of h = max(0, y), y ~ N(m, v), with v = v1 (v2 == NULL) or
 * v = v1 + v2:
 *   v > 0:   s = sqrtf(v);  al = m / s;  phi = 0.3989423f * expf(-0.5f * (al * al));  Phi = 0.5f * erfcf(-(al * 0.70710677f))
 *            a = max(m * Phi + s * phi, 0);   q = max((m * m + v) * Phi + (m * s) * phi, 0);   c = max(q - a * a, 0)
 *   else:    a = max(m, 0);  q = a * a;  c = 0        (zero inputs, pruned-away units, pad rows: no division, no NaN)
 * i.e. a = s (al Phi + phi), q = s^2 ((al^2 + 1) Phi + al phi) in the form that needs no al^2 (a huge |al| does not overflow);
 * Phi goes through erfcf on BOTH sides, so the lower tail keeps its relative accuracy; q - a * a is formed in fp32 before any
 * rounding to the operand type. a, q, c are PACKED operands (dtype, N x ld_out, each optional): pads are never written.
 * A streaming kernel, no LDS: a thread works 16 bytes of every output (4 fp32 / 8 bf16 columns) with 16-byte loads and stores
 * where the base addresses and leading dimensions allow (chosen per launch; a row's last partial group and everything else go
 * element by element, 4-byte loads). Bitwise reproducible (no reduction). m, v1, v2 are 4-byte aligned, a, q, c aligned to their
 * element; an output that overlaps an input or another output is VBNN_ERR_INVALID. */
typedef struct vbnn_relu_moments_args {
    const float* m; int64_t ld_m;           /* pre-activation mean, N x O fp32 */
    const float* v1; const float* v2; int64_t ld_v;   /* variance parts, N x O fp32 each (one ld); v2 may be NULL */
    int64_t N, O;
    void* a; void* q; void* c; int64_t ld_out;        /* E[h], E[h^2], Var[h]: packed (dtype), N x ld_out, ld_out >= O; NULL to skip */
} vbnn_relu_moments_args;
int vbnn_relu_moments(vbnn_ctx* ctx, int dtype, const vbnn_relu_moments_args* a);

/* dst[r][c] = T(float(src[r][c]) * float(src[r][c])) for r < rows, c < cols over a packed operand (dtype -> dtype; bf16: the
 * fp32 product rounded to nearest-even): the mu^2 operand from the mu shadow and the final Linear's w3^2 from its packed weight,
 * AS THEY ARE -- a dense pruned view's +0 entries, a held mask's, a compact network's shapes need nothing else. Pads are neither
 * read nor written. 16-byte accesses where both bases and both leading dimensions allow. */
int vbnn_square_shadow(vbnn_ctx* ctx, int dtype, const void* src, int64_t ld_src, int64_t rows, int64_t cols,
                       void* dst, int64_t ld_dst);

/* S draws of R x C Gaussian logits: y[s][r][c] = m[r][c] + sqrtf(v[r][c]) * z, z = lane c & 3 of
 * vbnn_normal4(seed, VBNN_STREAM_ZETA, layer, draw + s, row0 + r, c >> 2) -- the contract's bit-exact form (what
 * vbnn_fill_normal gives for the same address), one multiply and one add in fp32. `layer` is the FINAL Linear's layer id (the
 * number of VB layers): every other ZETA draw of the library belongs to a VB layer's forward (ids below it), and the final
 * Linear draws from EPS / ZETA nowhere else, so no existing path reads this stream. Draw s of row r starts at
 * y + s draw_stride + r ld_y: with ld_y = C, draw_stride = R C exactly the S R x C layout vbnn_predict_class_moments takes. */
typedef struct vbnn_logit_draws_args {
    const float* m; int64_t ld_m;           /* logit means, R x C fp32 */
    const float* v; int64_t ld_v;           /* logit variances, R x C fp32 (>= 0) */
    int64_t R, C, S;
    uint64_t seed; uint32_t layer; uint32_t draw; int64_t row0;
    float* y; int64_t ld_y; int64_t draw_stride;      /* ld_y >= C, draw_stride >= R ld_y */
} vbnn_logit_draws_args;
int vbnn_logit_draws(vbnn_ctx* ctx, const vbnn_logit_draws_args* a);

/* ---- signal-to-noise pruning (additive, ABI 6): mainviz.lua:20-27 on the device, and the pruned operand shadows that let
 * vbnn_forward / vbnn_head_predict evaluate the pruned network ---------------------------------------------------------------
 * The key of a weight is snr = |means / sqrt(exp(lvars))| in fp32, operation for operation as mainviz.lua:20 forms
 * torch.abs(torch.cdiv(means, torch.sqrt(vars))); all three calls below compute it with ONE device function, so a weight has
 * the same key bits in each. A NaN key (a NaN parameter, or 0 / 0: a zero mean under a variance that underflows to 0) orders
 * above every number and is never pruned. Denormals are not flushed: the key of a denormal mean at lvars = 0 is that denormal,
 * bit for bit, and a key that underflows is the correctly rounded denormal. A quiet NaN mean keeps its payload in the key
 * (fabsf clears the sign), a signalling one comes out quiet with the rest of its payload; the selection orders NaN keys by
 * their bit patterns, all of them above +inf.
 * Held by tests/test_prune_forms_gpu.py against tests/_prune_np.py: with v = the device's own fp32 expf(lvars) the key is bit
 * for bit fabsf(means / sqrtf(v)) (divide and square root correctly rounded), and within 2.25 ulp of |means| exp(-lvars / 2).
 * ALIGNMENT. None is required of any pointer or pitch below beyond the natural alignment of its element type; 16-byte
 * accesses are taken where the arguments allow them and the scalar paths leave the same bits. */
typedef struct vbnn_prune_desc {
    const float* means; const float* lvars; int64_t O, I;     /* the layer's fp32 parameters, O x I */
    /* vbnn_prune_pack only (vbnn_prune_select and vbnn_prune_workspace_bytes read the four fields above): */
    void* mu_p; void* var_p; int64_t ld_w;     /* pruned operand shadows, O x ld_w of dtype (allocate zeroed: pads are not written) */
    double* stats;                             /* 4 doubles, below */
    uint8_t* mask;                             /* optional O x I bytes, 1 = pruned (the `pruned` tensor of mainviz.lua:21); NULL to skip */
} vbnn_prune_desc;
/* mainviz.lua:20: snr_out[i] = the key of weight i (W floats): what nn.VBLinear exposes as :snr(). 16-byte loads and stores
 * when means, lvars and snr_out are all 16-byte aligned (the last W % 4 elements singly), 4-byte ones otherwise. */
int vbnn_snr(vbnn_ctx* ctx, const float* means, const float* lvars, int64_t W, float* snr_out);
/* mainviz.lua:20-21 turned round: tau_dev[0] = the EXACT k-th smallest key (0-based) over the union of the listed layers'
 * weights (n_layers <= 8; one layer = per-layer pruning, all of them = global), so that `key < tau` prunes at most k weights
 * (fewer when keys tie at tau). A radix select on the key's 32 bits (11 + 11 + 10): per digit one histogram sweep per layer
 * (integer counts: bitwise reproducible whatever the order of the atomics) and a one-workgroup kernel that picks the bin and
 * hands prefix and remaining rank to the next pass in device words. No host synchronisation, no allocation: the caller
 * passes `workspace` of at least vbnn_prune_workspace_bytes(...) bytes (4-byte aligned; contents irrelevant). Every pass
 * re-forms the keys from means / lvars (8 B per weight read, nothing per weight written). 0 <= k < W_total, else
 * VBNN_ERR_INVALID (to prune everything pass tau = +inf to vbnn_prune_pack). Fewer than 2^32 weights in all. A layer is read
 * with 16-byte loads when its means and lvars are both 16-byte aligned (whatever O and I: the layer is one run of O I
 * floats), with 4-byte loads otherwise. tau_dev[0] is the key's bit pattern, a NaN's payload included. */
int vbnn_prune_workspace_bytes(int n_layers, const vbnn_prune_desc* layers, size_t* bytes);
int vbnn_prune_select(vbnn_ctx* ctx, int n_layers, const vbnn_prune_desc* layers, int64_t k, float* tau_dev,
                      void* workspace, size_t workspace_bytes);
/* mainviz.lua:21-27: pruned = key < tau (strict, torch.lt) with tau = tau_dev[0] read on the device (chained behind
 * vbnn_prune_select without a host round trip), or tau_host when tau_dev is NULL. One sweep per layer and ONE finish kernel
 * for all layers (the shape of vbnn_prepare). Per layer: mu_p / var_p -- a kept weight's two values are bitwise what
 * vbnn_prepare writes to mu_s / var_s, a pruned weight's are +0 in both (no mean, no variance); stats[0..3] = { number
 * pruned, sum of exp(lvars) over the pruned weights, sum of exp(lvars) over all weights, W } -- pruned:sum(),
 * prunedvars:mean() W and vars:mean() W of mainviz.lua:22-27 -- from per-workgroup partials added in a fixed order (two
 * runs give the same bits); and optionally the byte mask. No transposed shadows: the predictive path is forward-only.
 * A NaN tau prunes nothing, tau = +inf everything but the NaN keys. ALIGNMENT, per layer: means / lvars take 16-byte loads
 * when I % 4 == 0 and both are 16-byte aligned; mu_p / var_p take 4-element stores when ld_w % 4 == 0 and both are 16-byte
 * aligned; the mask takes 4-byte stores when I % 4 == 0 and it is 4-byte aligned; element accesses otherwise, the same bits
 * either way. Pad elements (c >= I of a shadow row) are never written. */
int vbnn_prune_pack(vbnn_ctx* ctx, int dtype, int n_layers, const vbnn_prune_desc* layers, const float* tau_dev, float tau_host);

/* ---- compressed pruned weights and the forward that multiplies by them (additive, ABI 6) ------------------------------------
 * The pruned shadows above are dense: a network with 90 % of its weights pruned still streams every +0. The compressed form of
 * the same pruning keeps the KEPT weights only, per layer as CSR over output rows:
 *   row_ptr  O + 1 uint32: row o's entries are [row_ptr[o], row_ptr[o + 1]); row_ptr[0] = 0, row_ptr[O] = nnz
 *   cols     the entries' input units, ascending within a row; idx_bytes = 2 (uint16; I <= 65536 only) or 4 (uint32; any I)
 *   mu_v, var_v  the entries' two values in the packed dtype
 * An entry is a weight vbnn_prune_pack keeps -- !(key < tau) with the same key function and the same tau, so a NaN key is kept --
 * and its values are the bits vbnn_prune_pack stores for it, T(mean) and T(expf(lvar)): scattering the entries over +0 gives
 * mu_p / var_p bit for bit. A kept weight whose value is zero is still an entry: nnz = W - (number pruned), always. */
typedef struct vbnn_sparse_desc {
    uint32_t* row_ptr;                     /* O + 1 words */
    void* cols;                            /* nnz_cap indices of idx_bytes each */
    void* mu_v; void* var_v;               /* nnz_cap values of dtype each; var_v may be NULL (means only) */
    int64_t O, I;
    int64_t nnz_cap;                       /* entries the three arrays hold: nothing is written at or past it */
    uint32_t* nnz_dev;                     /* optional device word: the nnz this compress produced (= row_ptr[O]) */
    int32_t idx_bytes;                     /* 2 or 4; 2 with I > 65536 is VBNN_ERR_INVALID */
    int32_t reserved;
} vbnn_sparse_desc;
/* Builds the compressed form of layers[l] (its means, lvars, O, I are read; nothing else of the prune desc) into sparse[l], at
 * tau = tau_dev[0] read on the device (chained behind vbnn_prune_select like vbnn_prune_pack) or tau_host when tau_dev is NULL.
 * Per layer a count sweep (one wave per output row), ONE scan kernel for all layers (exclusive sums into row_ptr, nnz_dev) and
 * an ordered fill sweep (a wave walks its row in column order; an entry's place is its rank among the row's kept weights, from
 * a wave ballot): no atomics, no order dependence, two runs give the same bytes. No host synchronisation: the capacity is known
 * to a host that has read a vbnn_prune_pack's stats[0] for the same tau (nnz = W - pruned); with a smaller nnz_cap the entries
 * past it are dropped (row_ptr and nnz_dev still tell the true count, so the host can check). n_layers <= 8. Every access is
 * an element access: no alignment beyond the element types' is asked of any array. */
int vbnn_prune_compress(vbnn_ctx* ctx, int dtype, int n_layers, const vbnn_prune_desc* layers, const vbnn_sparse_desc* sparse,
                        const float* tau_dev, float tau_host);

/* One VB layer's updateOutput on compressed weights: m = x mu^T + b, v = (x.x)(sigma^2)^T, y = m + sqrt(v) . z -- the epilogue,
 * the noise addressing ((seed, ZETA, layer, draw, row0 + n, o >> 2), stacked draws by rows_per_draw; bf16 draws in the hardware
 * form, fp32 in the bit-exact form), ReLU and the packed outputs are vbnn_forward's own (one epilogue definition). var_v == NULL:
 * the single-product MAP form y = x mu^T + b. The input is K-MAJOR: xT (I x ld_xT, ld_xT >= N), the transpose vbnn_pack_input
 * (xT_s) and a forward's hT produce; x2T likewise, or NULL: the square is formed in registers as the packer stores it,
 * T(x . x) of the rounded x. A wave owns one output unit and 64 operand rows (a lane each): it walks the row's entries in
 * column order, each entry one coalesced read of xT[col][n .. n + 63], and adds in that order in fp32 -- bitwise reproducible.
 * Any N >= 1, O, I; rows without entries and nnz = 0 are fine. */
typedef struct vbnn_sparse_fwd_args {
    const uint32_t* row_ptr; const void* cols; const void* mu_v; const void* var_v;   /* as vbnn_sparse_desc */
    int64_t idx_bytes;
    const void* xT; const void* x2T; int64_t ld_xT;
    int64_t N, I, O;
    const float* bias;  /* O, may be NULL */
    uint64_t seed; uint32_t layer; uint32_t draw; int64_t row0;    /* LRT noise, as vbnn_fwd_args; ignored if var_v == NULL */
    /* outputs, each optional; meanings as in vbnn_fwd_args */
    float* y; int64_t ld_y;
    int64_t relu;
    void* h; void* h2; int64_t ld_h;       /* row-major N x ld_h (ld_h % 4 == 0): what the classifier head reads */
    void* hT; void* h2T; int64_t ld_hT;    /* K-major O x ld_hT: what the next sparse layer reads */
    int64_t rows_per_draw;
} vbnn_sparse_fwd_args;
int vbnn_forward_sparse(vbnn_ctx* ctx, int dtype, const vbnn_sparse_fwd_args* a);

/* ---- structured pruning: whole hidden units by signal-to-noise, and the compact network that is left (additive, ABI 6) ------
 * The group form of mainviz.lua:20-27. Unstructured pruning (above) leaves a network of the same shape; a hidden unit whose
 * incoming weights are all noise can go as a whole, and what remains is a smaller DENSE network for the ordinary kernels.
 * The key of output unit o of a VB layer is ||means[o, :]||_2 / ||sqrt(exp(lvars[o, :]))||_2 -- mainviz.lua:20's |mu| / sigma
 * when I = 1. None of the calls below synchronises or allocates. */
typedef struct vbnn_unit_desc {
    const float* means; const float* lvars; int64_t O, I;     /* the layer's fp32 parameters, O x I (read by vbnn_unit_snr only) */
    float* key;                                /* O floats: written by vbnn_unit_snr, read by vbnn_unit_select / vbnn_unit_index */
    uint32_t* keep;                            /* vbnn_unit_index: O words, the kept units ascending; the first n_keep[0] are written */
    uint32_t* n_keep;                          /* vbnn_unit_index: one device word, the length of the list */
} vbnn_unit_desc;
/* mainviz.lua:20 per unit: key[o] = sqrt(sum_i means[o,i]^2) / sqrt(sum_i expf(lvars[o,i])) for every listed layer. expf is the
 * weight key's (vbnn_snr); both sums run in double in one fixed order (a wave per row, or a workgroup per row when the rows are
 * few and long: wave shuffles, then the waves in order), square roots and quotient in double, ONE rounding to fp32: two runs give
 * the same bits. A NaN key (a NaN parameter, 0 / 0) is stored as the positive quiet NaN 0x7fc00000, so that keys order as their
 * bit patterns with NaN above every number; such a unit is never pruned. 8 B read per weight. n_layers <= 8.
 * A row is read with 16-byte loads when I % 4 == 0 and means and lvars are both 16-byte aligned, with 4-byte loads
 * otherwise; a thread adds the same elements in the same order either way, so the key does not depend on the alignment.
 * Held by tests/test_prune_forms_gpu.py: the key is float32(sqrt(sum m^2) / sqrt(sum v)) evaluated in double from the device's
 * own v = expf(lvars), exactly, wherever the order of the double additions cannot move the quotient across a rounding
 * midpoint. */
int vbnn_unit_snr(vbnn_ctx* ctx, int n_layers, const vbnn_unit_desc* layers);
/* mainviz.lua:20-21 turned round, per unit: tau = the EXACT k-th smallest key (0-based) over the union of the listed layers'
 * units, read from the key arrays vbnn_unit_snr wrote, so that `key < tau` prunes at most k units (fewer when keys tie at tau)
 * -- what vbnn_prune_select is for weights. It is written to tau_dev[0 .. n_layers), one copy per listed layer: the array
 * vbnn_unit_index reads (all layers in one call = one global threshold; a call per layer with tau_dev + l = one per layer). One
 * one-workgroup kernel (a radix select on the 32 key bits, integer counts). 0 <= k < n_units, else VBNN_ERR_INVALID (to prune
 * everything pass tau = +inf to vbnn_unit_index). */
int vbnn_unit_select(vbnn_ctx* ctx, int n_layers, const vbnn_unit_desc* layers, int64_t k, float* tau_dev);
/* mainviz.lua:21 per unit, as index lists: layer l's threshold is tau_dev[l] read on the device (an array of n_layers floats,
 * chained behind vbnn_unit_select), or tau_host for every layer when tau_dev is NULL. With n0 = #{o : !(key[o] < tau)} and
 * n = min(O, multiple ceil(max(n0, 1) / multiple)), the kept set is the n units that come first in the order "larger key first,
 * NaN above all numbers, on equal keys the lower index first": with multiple = 1 and n0 >= 1 exactly {o : !(key[o] < tau)}; a
 * layer that would lose every unit keeps its best one; multiple = 256 gives widths the tiled GEMM kernels take. keep[0 .. n) =
 * the kept units ascending, n_keep[0] = n. One workgroup per layer; places come from ordered counts (wave ballots): no atomics
 * on the list, two runs give the same words. multiple >= 1. */
int vbnn_unit_index(vbnn_ctx* ctx, int n_layers, const vbnn_unit_desc* layers, const float* tau_dev, float tau_host, int64_t multiple);
/* The compaction: dst_means[r, c] = means[rows[r], cols[c]], dst_lvars likewise in the same sweep, dst_bias[r] = bias[rows[r]] --
 * fp32 bit copies into dense n_rows x n_cols arrays. rows == NULL: every row (n_rows = O); cols == NULL: every column
 * (n_cols = I). lvars / dst_lvars and bias / dst_bias are optional, in pairs: a VB layer passes all three (rows = its own kept
 * list, cols = the previous layer's), the final Linear its weight alone with cols = the last VB layer's list. The list LENGTHS
 * are host values (read back from n_keep). Index words are clamped to the source shape (a word >= O reads row O - 1, a word
 * >= I column I - 1). Any O, I, n_rows, n_cols >= 1. dst_means / dst_lvars take 16-byte stores when n_cols % 4 == 0 and both
 * are 16-byte aligned; without a column list the source takes 16-byte loads when I % 4 == 0 and means / lvars are 16-byte
 * aligned; element accesses otherwise. Nothing behind n_rows x n_cols (or n_rows) elements is written. */
typedef struct vbnn_unit_gather_args {
    const float* means; const float* lvars; const float* bias; int64_t O, I;      /* source: O x I (and O) */
    const uint32_t* rows; int64_t n_rows;
    const uint32_t* cols; int64_t n_cols;
    float* dst_means; float* dst_lvars; float* dst_bias;                           /* n_rows x n_cols (and n_rows) */
} vbnn_unit_gather_args;
int vbnn_unit_gather(vbnn_ctx* ctx, const vbnn_unit_gather_args* a);

/* ---- a device digest of a buffer (additive, ABI 6): what a checkpoint records per tensor before the download and checks again
 * after the upload, and what the replicas of a data-parallel run compare in 8 bytes per tensor -------------------------------
 * Over the buffer's 32-bit words w_0 .. w_{n_words - 1} (little-endian, as they lie in memory; the bits of a float, NaN
 * payloads and the sign of a zero included):
 *   out[0] += sum_i mix(((index0 + i + 1) << 32) | w_i)   mod 2^64
 * with mix the splitmix64 finaliser on a uint64 z, every operation mod 2^64:
 *   z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z = z ^ (z >> 31)
 * Position-dependent (two unequal words swapped change it) and order-independent (a sum of integers): any grid and any order of
 * the atomics give the same bits, and the digests of the pieces of a buffer, each taken with index0 = the piece's first word,
 * add up to the digest of the whole. The call ADDS into out (a device word, 8-byte aligned): the caller zeroes it, and several
 * calls may accumulate into one word. It detects damage; it is NOT cryptographic -- anyone can construct a collision.
 * VBNN_ERR_INVALID, with out untouched: index0 + n_words > 2^32 - 1, buf not 4-byte aligned, out NULL. n_words = 0 is legal and
 * adds nothing (buf is then not read and may be NULL). One read-only streaming launch: 16-byte loads on the 16-byte aligned
 * body, 4-byte loads for a head and a tail of up to three words each, one 64-bit integer atomic per workgroup; no floating-point
 * arithmetic. 4 B read per word, nothing written. */
int vbnn_digest(vbnn_ctx* ctx, const void* buf, uint64_t n_words, uint64_t index0, uint64_t* out);

/* The same criterion as separate modules, for the module-level call order of mlp.lua:77-80:
 * nn.LogSoftMax:updateOutput is vbnn_logsoftmax_nll with g_logits = loss = correct = NULL. Both clamp a target outside
 * [0, C - 1] into it, as vbnn_logsoftmax_nll does: the row that vbnn_nll_forward charges to class 0 or C - 1 gets its
 * gradient -inv_n at that same class from vbnn_nll_backward. loss_sum_dev / correct_dev are ADDED to (the caller clears them). */
int vbnn_nll_forward(vbnn_ctx* ctx, const float* out, int64_t ld, const int32_t* target, int64_t N, int64_t C,
                     float inv_n, double* loss_sum_dev, int32_t* correct_dev);          /* criterion:forward  */
int vbnn_nll_backward(vbnn_ctx* ctx, const int32_t* target, int64_t N, int64_t C, float inv_n, float* g); /* :backward */
int vbnn_logsoftmax_backward(vbnn_ctx* ctx, const float* out, const float* g, float* gx, int64_t N, int64_t C);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* VBNN_HIP_H */
