// gemm_chain.hip -- vbnn_backward_chain: updateGradInput and accGradParameters of ONE layer as one launch of the two-pass 256 x 256
// kernel (gemm_v3.h, gemm_nt_v3_chain), for the bf16 layers whose two gradients each take that kernel's plain K-major form on their
// own; otherwise exactly the two calls. (A translation unit of its own: it instantiates the kernel bodies of both functors.)
#include "gemm_dispatch.h"

// would vbnn_grad_input / vbnn_acc_grad_parameters send these blocks to launch_gemm_v3<true, true, false, EpiDx> /
// <true, true, true, EpiDw>? The conditions of grad_input_t, acc_grad_t and try_kmajor, restated in their order.
static bool chain_dx_ok(const vbnn_dx_args* a, const EpiDx<bf16_t>& e) {
    return a->gv && a->w && a->w2 && a->g && !a->gT_prev && !a->gvT_prev && kmajor_selected(a->I, a->N, a->O) &&
           gemm_v3_possible(a->I, a->N, a->O, a->ld_w, a->ld_g, true, false, e);
}
static bool chain_dw_ok(const vbnn_dw_args* a, const EpiDw& e) {
    if (a->part != 0 || a->accumulate != 0 || !e.lrt || a->gradBias || e.has_draw_dev()) return false;
    if (!a->x || !a->x2 || !a->g || !a->gv) return false;
    if (a->gT && a->gvT && g_kmajor) return false;           // (the mixed form comes first in acc_grad_t: not chained)
    return kmajor_selected(a->I, a->O, a->N) && gemm_v3_possible(a->I, a->O, a->N, a->ld_x, a->ld_g, true, true, e);
}

extern "C" int vbnn_backward_chain(vbnn_ctx* ctx, int dtype, const vbnn_dx_args* dx, const vbnn_dw_args* dw, int order) {
    VBNN_API_BEGIN
    vbnn_cu_scope plan(ctx);                                 // shape heuristics: this context's compute units
    int chk = check_dx_args(ctx, dx);
    if (chk != VBNN_OK) return chk;
    chk = check_dw_args(ctx, dtype, dw);
    if (chk != VBNN_OK) return chk;
    VBNN_REQUIRE(dx->N == dw->N && dx->I == dw->I && dx->O == dw->O, "the two argument blocks describe one layer");
    VBNN_REQUIRE(order == VBNN_CHAIN_DX_FIRST || order == VBNN_CHAIN_DW_FIRST, "order: VBNN_CHAIN_DX_FIRST or VBNN_CHAIN_DW_FIRST");
    g_v3_last_chained = 0;
    if (dtype == VBNN_BF16 && !g_v3_chain_off) {
        const EpiDx<bf16_t> ex = make_dx_epi<bf16_t>(dx);
        const EpiDw ew = make_dw_epi<bf16_t>(dw);
        if (chain_dx_ok(dx, ex) && chain_dw_ok(dw, ew)) {
            const bf16_t* w = (const bf16_t*)dx->w;  const bf16_t* w2 = (const bf16_t*)dx->w2;
            const bf16_t* g = (const bf16_t*)dx->g;  const bf16_t* gv = (const bf16_t*)dx->gv;
            const bf16_t* x = (const bf16_t*)dw->x;  const bf16_t* x2 = (const bf16_t*)dw->x2;
            const bf16_t* h = (const bf16_t*)dw->g;  const bf16_t* hv = (const bf16_t*)dw->gv;
            int st;
            if (order == VBNN_CHAIN_DX_FIRST)
                st = launch_gemm_v3_chain<bf16_t, true, false, EpiDx<bf16_t>, true, true, EpiDw>(
                    ctx, w, w2, dx->ld_w, g, gv, dx->ld_g, (int)dx->I, (int)dx->N, (int)dx->O, ex,
                    x, x2, dw->ld_x, h, hv, dw->ld_g, (int)dw->I, (int)dw->O, (int)dw->N, ew);
            else
                st = launch_gemm_v3_chain<bf16_t, true, true, EpiDw, true, false, EpiDx<bf16_t>>(
                    ctx, x, x2, dw->ld_x, h, hv, dw->ld_g, (int)dw->I, (int)dw->O, (int)dw->N, ew,
                    w, w2, dx->ld_w, g, gv, dx->ld_g, (int)dx->I, (int)dx->N, (int)dx->O, ex);
            if (st == VBNN_OK) g_v3_last_chained = 1;
            if (st != VBNN_ERR_UNSUPPORTED) return st;
        }
    }
    if (order == VBNN_CHAIN_DX_FIRST) {
        const int st = vbnn_grad_input(ctx, dtype, dx);
        if (st != VBNN_OK) return st;
        return vbnn_acc_grad_parameters(ctx, dtype, dw);
    }
    const int st = vbnn_acc_grad_parameters(ctx, dtype, dw);
    if (st != VBNN_OK) return st;
    return vbnn_grad_input(ctx, dtype, dx);
    VBNN_API_END
}
