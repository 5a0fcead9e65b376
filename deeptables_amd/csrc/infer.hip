// infer.hip — the host side of every fused inference plan: dt_deepfm_infer*, dt_dcn_infer*, dt_stack_infer* and
// dt_xdeepfm_infer* (include/dt_hip.h).  The kernels are in infer_x3.h; the train step is deepfm.hip.
#include "infer_x3.h"

using namespace dt;

// ---- DeepFM / DCN / net-stack inference (infer_x3.h): one k_infer (or, without a tower, k_infer_sparse) launch per batch
//      over the layouts one k_infer_prep launch wrote ----
static bool infer_tower_ok(int H1, int H2, int cells) {
    return H1 >= 1 && H1 <= kH1 && H2 >= 1 && H2 <= kH2 && (cells & ~3) == 0;
}

extern "C" int dt_deepfm_infer_supported(int F, int D, int Nd, int H1, int H2, int cells) {
    DeepFmDims dm; int lpr;
    return (infer_tower_ok(H1, H2, cells) && deepfm_dims(1, F, D, Nd, &dm, &lpr) &&
            infer_lds_bytes(dm.CP, false) <= 160 * 1024) ? 1 : 0;
}

extern "C" int dt_dcn_infer_supported(int F, int D, int Nd, int H1, int H2, int cells, int L) {
    DeepFmDims dm; int lpr;
    return (infer_tower_ok(H1, H2, cells) && L >= 1 && L <= kCrossMax && deepfm_dims(1, F, D, Nd, &dm, &lpr) &&
            infer_lds_bytes(dm.CP, true) <= 160 * 1024) ? 1 : 0;
}

extern "C" int64_t dt_deepfm_infer_workspace_bytes(int F, int D, int Nd) {
    DeepFmDims dm; int lpr;
    if (!deepfm_dims(1, F, D, Nd, &dm, &lpr)) return -1;
    return infer_ws_layout(dm.CP, 0, kNetAll).total * (int64_t)sizeof(float);
}

extern "C" int64_t dt_dcn_infer_workspace_bytes(int F, int D, int Nd, int L) {
    DeepFmDims dm; int lpr;
    if (!deepfm_dims(1, F, D, Nd, &dm, &lpr) || L < 1 || L > kCrossMax) return -1;
    return infer_ws_layout(dm.CP, L, DT_NET_DNN).total * (int64_t)sizeof(float);
}

static int infer_prepare(const char* what, int F, int D, int Nd, InferPrepArgs a, int cells, void* workspace, void* stream) {
    DeepFmDims dm; int lpr;
    DT_UNSUPPORTED(!deepfm_dims(1, F, D, Nd, &dm, &lpr), "%s: unsupported shape F=%d D=%d Nd=%d", what, F, D, Nd);
    const bool tower = (a.nets & DT_NET_DNN) != 0, lin = (a.nets & DT_NET_LINEAR) != 0;
    if (tower) {
        DT_UNSUPPORTED(!infer_tower_ok(a.H1, a.H2, cells), "%s: tower %d x %d, cells %d (H1 <= %d, H2 <= %d, cells: BN bits 0 / 1)",
                       what, a.H1, a.H2, cells, kH1, kH2);
        DT_REQUIRE(a.ld1 >= a.H1 && a.ld2 >= a.H2, "%s: leading dimensions ld1=%d ld2=%d below the widths", what, a.ld1, a.ld2);
    }
    // w_out may be missing (= 1) only where the tower's vector is task_output's own kernel: DCN and the tower alone
    DT_REQUIRE(workspace && (!tower || (a.mm && a.mv && a.W1 && a.W2 && a.w3)) && (!lin || a.wlin) &&
               (a.L > 0 || a.nets == DT_NET_DNN || a.wout), "%s: null pointer", what);
    DT_REQUIRE(a.L == 0 || (a.cw && a.cb_), "%s: null cross weights", what);
    if (tower) {
        if (const int rc = infer_check_cells(what, cells, a.cm, a.cv)) return rc;
    }
    DT_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", what);
    const int items = tower ? max((dm.CP >> 5) * 512, (2 * a.L + 1) * dm.CP) : dm.CP;
    hipLaunchKernelGGL(k_infer_prep, dim3(ceil_div(items, 256)), dim3(256), 0, as_stream(stream), dm, a,
                       reinterpret_cast<float*>(workspace));
    return launch_status(what);
}

extern "C" int dt_deepfm_infer_prepare(int F, int D, int Nd, const float* w_lin, const float* bn_gamma, const float* bn_beta,
                                       const float* bn_mean, const float* bn_var, float bn_eps, const float* W1, int ld1,
                                       int H1, const float* b1, const float* W2, int ld2, int H2, const float* b2, int cells,
                                       const float* c1_gamma, const float* c1_beta, const float* c1_mean, const float* c1_var,
                                       float c1_eps, const float* c2_gamma, const float* c2_beta, const float* c2_mean,
                                       const float* c2_var, float c2_eps, const float* w3, const float* w_out,
                                       const float* b_out, void* workspace, void* stream) {
    const InferPrepArgs a{w_lin, bn_gamma, bn_beta, bn_mean, bn_var, bn_eps, W1, ld1, H1, W2, ld2, H2,
                          {b1, b2}, {c1_gamma, c2_gamma}, {c1_beta, c2_beta}, {c1_mean, c2_mean}, {c1_var, c2_var},
                          {c1_eps, c2_eps}, w3, w_out, b_out, nullptr, nullptr, 0, kNetAll};
    return infer_prepare("dt_deepfm_infer_prepare", F, D, Nd, a, cells, workspace, stream);
}

extern "C" int dt_dcn_infer_prepare(int F, int D, int Nd, const float* cross_w, const float* cross_b, int L,
                                    const float* bn_gamma, const float* bn_beta, const float* bn_mean, const float* bn_var,
                                    float bn_eps, const float* W1, int ld1, int H1, const float* b1, const float* W2, int ld2,
                                    int H2, const float* b2, int cells, const float* c1_gamma, const float* c1_beta,
                                    const float* c1_mean, const float* c1_var, float c1_eps, const float* c2_gamma,
                                    const float* c2_beta, const float* c2_mean, const float* c2_var, float c2_eps,
                                    const float* w3, const float* w_out, const float* b_out, void* workspace, void* stream) {
    DT_UNSUPPORTED(L < 1 || L > kCrossMax, "dt_dcn_infer_prepare: %d cross layers (1..%d)", L, kCrossMax);
    const InferPrepArgs a{nullptr, bn_gamma, bn_beta, bn_mean, bn_var, bn_eps, W1, ld1, H1, W2, ld2, H2,
                          {b1, b2}, {c1_gamma, c2_gamma}, {c1_beta, c2_beta}, {c1_mean, c2_mean}, {c1_var, c2_var},
                          {c1_eps, c2_eps}, w3, w_out, b_out, cross_w, cross_b, L, DT_NET_DNN};
    return infer_prepare("dt_dcn_infer_prepare", F, D, Nd, a, cells, workspace, stream);
}

static int infer_run(const char* what, const void* idx, int idx_kind, const float* table, const int64_t* row_offset,
                     const int32_t* vocab, const float* dense, int B, int F, int D, int Nd, int L, const void* workspace,
                     float* logit_out, float* out, int* oob_count, int flags, void* stream, int nets = kNetAll,
                     float* xd_x0 = nullptr) {
    // xd_x0 != NULL: xDeepFM's tower launch (nets = DT_NET_LINEAR | DT_NET_DNN) — the gathered rows go to xd_x0 and logit_out
    // receives linear + tower . w3 (k_infer's XD variant)
    DT_REQUIRE(B >= 0, "%s: B=%d", what, B);
    DeepFmDims dm; int lpr;
    DT_UNSUPPORTED(!deepfm_dims(1, F, D, Nd, &dm, &lpr), "%s: unsupported shape F=%d D=%d Nd=%d", what, F, D, Nd);
    DT_REQUIRE((flags & ~(DT_INFER_SIGMOID | DT_INFER_TOWER_BF16)) == 0, "%s: flags 0x%x", what, flags);
    DT_REQUIRE(idx_kind == DT_IDX_F32 || idx_kind == DT_IDX_I32, "%s: idx_kind %d", what, idx_kind);
    if (B == 0) return DT_OK;
    if (const int rc = infer_check_io(what, idx, table, row_offset, vocab, workspace, logit_out, Nd == 0 || dense)) return rc;
    dm.B = B;
    const bool dcn = L > 0, one = (flags & DT_INFER_TOWER_BF16) != 0;
    const bool xd = xd_x0 != nullptr;
    DT_REQUIRE(!xd || (uintptr_t)xd_x0 % 16 == 0, "%s: x0_out must be 16-byte aligned", what);
    const InferIo io{idx, idx_kind, reinterpret_cast<const float4*>(table), row_offset, vocab, dense, logit_out, out, oob_count,
                     (flags & DT_INFER_SIGMOID) ? 1 : 0, reinterpret_cast<float4*>(xd_x0), xd ? logit_out : nullptr};
    const float* ws = reinterpret_cast<const float*>(workspace);
    hipStream_t st = as_stream(stream);
    if (!(nets & DT_NET_DNN)) {     // no tower: one wave per row, no LDS (the precision flag has nothing to act on)
        const dim3 grid(ceil_div(B, kInferSparseRows)), block(64 * kInferSparseRows);
        switch (nets) {
            case DT_NET_LINEAR: hipLaunchKernelGGL((k_infer_sparse<DT_NET_LINEAR>), grid, block, 0, st, io, dm, ws); break;
            case DT_NET_FM: hipLaunchKernelGGL((k_infer_sparse<DT_NET_FM>), grid, block, 0, st, io, dm, ws); break;
            default: hipLaunchKernelGGL((k_infer_sparse<DT_NET_LINEAR | DT_NET_FM>), grid, block, 0, st, io, dm, ws); break;
        }
        return launch_status(what);
    }
    const size_t lds = infer_lds_bytes(dm.CP, dcn);
    DT_UNSUPPORTED(lds > 160 * 1024, "%s: the tile needs %zu B of LDS", what, lds);
    const int tiles = ceil_div(B, kTM);
#define DT_IL(N, LCV, ONEV, NETS)                                                                                          \
    do {                                                                                                                   \
        hipFuncSetAttribute((const void*)k_infer<N, LCV, ONEV, NETS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        hipLaunchKernelGGL((k_infer<N, LCV, ONEV, NETS>), dim3(tiles), dim3(kInferThreads), lds, st, io, dm, ws, L);        \
    } while (0)
#define DT_IM(N, NETS)                                                                                               \
    case NETS:                                                                                                       \
        if (one) DT_IL(N, 0, true, NETS); else DT_IL(N, 0, false, NETS);                                             \
        break;
#define DT_IX(N)                                                                                                     \
    do {                                                                                                             \
        constexpr int XN = DT_NET_DNN | DT_NET_LINEAR;                                                               \
        if (one) {                                                                                                   \
            hipFuncSetAttribute((const void*)k_infer<N, 0, true, XN, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            hipLaunchKernelGGL((k_infer<N, 0, true, XN, true>), dim3(tiles), dim3(kInferThreads), lds, st, io, dm, ws, L);        \
        } else {                                                                                                     \
            hipFuncSetAttribute((const void*)k_infer<N, 0, false, XN, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            hipLaunchKernelGGL((k_infer<N, 0, false, XN, true>), dim3(tiles), dim3(kInferThreads), lds, st, io, dm, ws, L);       \
        }                                                                                                            \
    } while (0)
#define DT_IN(N)                                                                                                     \
    case N:                                                                                                          \
        if (xd) DT_IX(N);                                                                                            \
        else if (dcn) { if (one) DT_IL(N, kCrossMax, true, kNetAll); else DT_IL(N, kCrossMax, false, kNetAll); }          \
        else switch (nets) {                                                                                         \
            DT_IM(N, DT_NET_DNN) DT_IM(N, DT_NET_DNN | DT_NET_LINEAR) DT_IM(N, DT_NET_DNN | DT_NET_FM) DT_IM(N, kNetAll) \
        }                                                                                                            \
        break;
    switch (dm.CP >> 6) { DT_IN(1) DT_IN(2) DT_IN(3) DT_IN(4) DT_IN(5) DT_IN(6) DT_IN(7) DT_IN(8) DT_IN(9) }
#undef DT_IN
#undef DT_IX
#undef DT_IM
#undef DT_IL
    return launch_status(what);
}

extern "C" int dt_deepfm_infer(const void* idx, int idx_kind, const float* table, const int64_t* row_offset,
                               const int32_t* vocab, const float* dense, int B, int F, int D, int Nd, const void* workspace,
                               float* logit_out, float* out, int* oob_count, int flags, void* stream) {
    return infer_run("dt_deepfm_infer", idx, idx_kind, table, row_offset, vocab, dense, B, F, D, Nd, 0, workspace, logit_out,
                     out, oob_count, flags, stream);
}

extern "C" int dt_dcn_infer(const void* idx, int idx_kind, const float* table, const int64_t* row_offset,
                            const int32_t* vocab, const float* dense, int B, int F, int D, int Nd, int L,
                            const void* workspace, float* logit_out, float* out, int* oob_count, int flags, void* stream) {
    DT_UNSUPPORTED(L < 1 || L > kCrossMax, "dt_dcn_infer: %d cross layers (1..%d)", L, kCrossMax);
    return infer_run("dt_dcn_infer", idx, idx_kind, table, row_offset, vocab, dense, B, F, D, Nd, L, workspace, logit_out,
                     out, oob_count, flags, stream);
}

// ---- every Add-stacked subset of {linear, fm_nets, dnn_nets} (reference deepmodel.py:286-301: the nets' logits, Add,
//      task_output; deepnets.py:43-66 linear, 84-96 fm_nets, 163-169 dnn_nets) through the same launches ----
static bool stack_nets_ok(int nets) { return nets >= 1 && nets <= kNetAll; }

extern "C" int dt_stack_infer_supported(int F, int D, int Nd, int H1, int H2, int cells, int nets) {
    DeepFmDims dm; int lpr;
    if (!stack_nets_ok(nets) || !deepfm_dims(1, F, D, Nd, &dm, &lpr)) return 0;
    if (!(nets & DT_NET_DNN)) return 1;
    return (infer_tower_ok(H1, H2, cells) && infer_lds_bytes(dm.CP, false) <= 160 * 1024) ? 1 : 0;
}

extern "C" int64_t dt_stack_infer_workspace_bytes(int F, int D, int Nd, int nets) {
    DeepFmDims dm; int lpr;
    if (!stack_nets_ok(nets) || !deepfm_dims(1, F, D, Nd, &dm, &lpr)) return -1;
    return infer_ws_layout(dm.CP, 0, nets).total * (int64_t)sizeof(float);
}

extern "C" int dt_stack_infer_prepare(int F, int D, int Nd, int nets, const float* w_lin, const float* bn_gamma,
                                      const float* bn_beta, const float* bn_mean, const float* bn_var, float bn_eps,
                                      const float* W1, int ld1, int H1, const float* b1, const float* W2, int ld2, int H2,
                                      const float* b2, int cells, const float* c1_gamma, const float* c1_beta,
                                      const float* c1_mean, const float* c1_var, float c1_eps, const float* c2_gamma,
                                      const float* c2_beta, const float* c2_mean, const float* c2_var, float c2_eps,
                                      const float* w3, const float* w_out, const float* b_out, void* workspace, void* stream) {
    DT_REQUIRE(stack_nets_ok(nets), "dt_stack_infer_prepare: nets 0x%x (a non-empty mask of DT_NET_LINEAR | DT_NET_FM | DT_NET_DNN)", nets);
    DT_REQUIRE(!(nets & DT_NET_LINEAR) || w_lin, "dt_stack_infer_prepare: nets 0x%x has linear but w_lin is null", nets);
    DT_REQUIRE(!(nets & DT_NET_DNN) || (bn_mean && bn_var && W1 && W2 && w3),
               "dt_stack_infer_prepare: nets 0x%x has dnn_nets but a tower pointer (bn_mean, bn_var, W1, W2, w3) is null", nets);
    DT_REQUIRE(nets == DT_NET_DNN || w_out, "dt_stack_infer_prepare: nets 0x%x needs w_out (null only for dnn_nets alone)", nets);
    const InferPrepArgs a{w_lin, bn_gamma, bn_beta, bn_mean, bn_var, bn_eps, W1, ld1, H1, W2, ld2, H2,
                          {b1, b2}, {c1_gamma, c2_gamma}, {c1_beta, c2_beta}, {c1_mean, c2_mean}, {c1_var, c2_var},
                          {c1_eps, c2_eps}, w3, w_out, b_out, nullptr, nullptr, 0, nets};
    return infer_prepare("dt_stack_infer_prepare", F, D, Nd, a, cells, workspace, stream);
}

extern "C" int dt_stack_infer(const void* idx, int idx_kind, const float* table, const int64_t* row_offset,
                              const int32_t* vocab, const float* dense, int B, int F, int D, int Nd, int nets, const void* workspace,
                              float* logit_out, float* out, int* oob_count, int flags, void* stream) {
    DT_REQUIRE(stack_nets_ok(nets), "dt_stack_infer: nets 0x%x (a non-empty mask of DT_NET_LINEAR | DT_NET_FM | DT_NET_DNN)", nets);
    return infer_run("dt_stack_infer", idx, idx_kind, table, row_offset, vocab, dense, B, F, D, Nd, 0, workspace, logit_out,
                     out, oob_count, flags, stream, nets);
}

// ---- xDeepFM inference (nets 'linear' + 'cin_nets' + 'dnn_nets', Add-stacked; reference deepnets.py:43-81 + 163-169,
//      layers.py:638-734, deepmodel.py:286-301): 2 + n launches per batch over a workspace written once —
//      k_infer<XD> (gather once; linear + tower -> partial, the raw rows -> x0), one CIN layer kernel per layer on the
//      filter dt_cin_pack wrote, k_xdeepfm_head (pool, exFM_out, Add, task_output, activation). ----
constexpr int kXdNets = DT_NET_LINEAR | DT_NET_DNN;

struct XdLayout {
    int n;
    int L[kXdMaxLayers], Hk[kXdMaxLayers], lo[kXdMaxLayers], woff[kXdMaxLayers];
    int P;                               // pooled channels = exFM_out's inputs
    int64_t wex;                         // floats: exFM_out's kernel [P rounded up to 4] | its bias [4]
    int64_t filt[kXdMaxLayers];          // bytes: layer k's packed filter (dt_cin_pack)
    int64_t total;                       // bytes
};

// the layers' shapes (layers.py:655-687: direct=False halves every layer but the last) and the workspace behind the tower's
// layouts; false when the CIN is outside what the launches take
static bool xd_layout(int F, int CP, int n, const int* sizes, int direct, int mode, XdLayout* x) {
    if (n < 1 || n > kXdMaxLayers || !sizes || F < 1 || F > 64) return false;
    if (mode != DT_CIN_F32 && mode != DT_CIN_BF16 && mode != DT_CIN_BF16X3) return false;
    x->n = n;
    x->P = 0;
    int hk = F;
    for (int k = 0; k < n; ++k) {
        const int Lk = sizes[k];
        if (Lk < 1) return false;
        const bool last = k == n - 1;
        if (!direct && !last && (Lk & 1)) return false;
        x->L[k] = Lk; x->Hk[k] = hk;
        x->lo[k] = (direct || last) ? 0 : Lk / 2;
        x->woff[k] = x->P;
        x->P += Lk - x->lo[k];
        hk = direct ? Lk : Lk / 2;
    }
    int64_t o = infer_ws_layout(CP, 0, kXdNets).total * (int64_t)sizeof(float);
    x->wex = o / (int64_t)sizeof(float);
    o += (((int64_t)x->P + 3) & ~(int64_t)3) * 4 + 16;
    for (int k = 0; k < n; ++k) {
        const int64_t nb = dt_cin_packed_bytes(mode, F, x->Hk[k], x->L[k]);
        if (nb < 0) return false;
        x->filt[k] = o;
        o += nb;
    }
    x->total = o;
    return true;
}

extern "C" int dt_xdeepfm_infer_supported(int F, int D, int Nd, int H1, int H2, int cells, int n_layers, const int* layer_sizes,
                                          int direct, int use_residual, int reduce_D, int act, int cin_mode) {
    DeepFmDims dm; int lpr;
    XdLayout x;
    if (use_residual || reduce_D || !dt_stack_infer_supported(F, D, Nd, H1, H2, cells, kXdNets)) return 0;
    if (!deepfm_dims(1, F, D, Nd, &dm, &lpr) || !xd_layout(F, dm.CP, n_layers, layer_sizes, direct, cin_mode, &x)) return 0;
    for (int k = 0; k < x.n; ++k)
        if (!dt_cin_fwd_supported(cin_mode, F, x.Hk[k], x.L[k], D, act)) return 0;
    return 1;
}

extern "C" int64_t dt_xdeepfm_infer_workspace_bytes(int F, int D, int Nd, int n_layers, const int* layer_sizes, int direct,
                                                    int cin_mode) {
    DeepFmDims dm; int lpr;
    XdLayout x;
    if (!deepfm_dims(1, F, D, Nd, &dm, &lpr) || !xd_layout(F, dm.CP, n_layers, layer_sizes, direct, cin_mode, &x)) return -1;
    return x.total;
}

extern "C" int dt_xdeepfm_infer_prepare(int F, int D, int Nd, const float* w_lin, const float* bn_gamma, const float* bn_beta,
                                        const float* bn_mean, const float* bn_var, float bn_eps, const float* W1, int ld1,
                                        int H1, const float* b1, const float* W2, int ld2, int H2, const float* b2, int cells,
                                        const float* c1_gamma, const float* c1_beta, const float* c1_mean, const float* c1_var,
                                        float c1_eps, const float* c2_gamma, const float* c2_beta, const float* c2_mean,
                                        const float* c2_var, float c2_eps, const float* w3, const float* w_out,
                                        const float* b_out, int n_layers, const int* layer_sizes, int direct, int cin_mode,
                                        const float* const* cin_W, const float* w_ex, const float* b_ex, void* workspace,
                                        void* stream) {
    const char* who = "dt_xdeepfm_infer_prepare";
    DeepFmDims dm; int lpr;
    XdLayout x;
    DT_UNSUPPORTED(!deepfm_dims(1, F, D, Nd, &dm, &lpr), "%s: unsupported shape F=%d D=%d Nd=%d", who, F, D, Nd);
    DT_UNSUPPORTED(!xd_layout(F, dm.CP, n_layers, layer_sizes, direct, cin_mode, &x),
                   "%s: CIN of %d layers, mode %d, F=%d (1..%d layers of >= 1 filters, even but the last with direct=0; F <= 64)",
                   who, n_layers, cin_mode, F, kXdMaxLayers);
    DT_REQUIRE(w_lin && w3 && w_out && cin_W && w_ex, "%s: null pointer (w_lin, w3, w_out, cin_W, w_ex)", who);
    for (int k = 0; k < x.n; ++k) DT_REQUIRE(cin_W[k], "%s: cin_W[%d] is null", who, k);
    const InferPrepArgs a{w_lin, bn_gamma, bn_beta, bn_mean, bn_var, bn_eps, W1, ld1, H1, W2, ld2, H2,
                          {b1, b2}, {c1_gamma, c2_gamma}, {c1_beta, c2_beta}, {c1_mean, c2_mean}, {c1_var, c2_var},
                          {c1_eps, c2_eps}, w3, w_out, b_out, nullptr, nullptr, 0, kXdNets};
    int rc = infer_prepare(who, F, D, Nd, a, cells, workspace, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_xdeepfm_prep, dim3(ceil_div(x.P + 1, 256)), dim3(256), 0, as_stream(stream), w_ex, b_ex, x.P,
                       reinterpret_cast<float*>(workspace) + x.wex);
    rc = launch_status(who);
    for (int k = 0; k < x.n && !rc; ++k)
        rc = dt_cin_pack(cin_mode, cin_W[k], F, x.Hk[k], x.L[k], reinterpret_cast<char*>(workspace) + x.filt[k], stream);
    return rc;
}

extern "C" int dt_xdeepfm_infer_tower(const void* idx, int idx_kind, const float* table, const int64_t* row_offset,
                                      const int32_t* vocab, const float* dense, int B, int F, int D, int Nd,
                                      const void* workspace, float* x0_out, float* partial_out, int* oob_count, int flags,
                                      void* stream) {
    DT_REQUIRE((flags & ~DT_INFER_TOWER_BF16) == 0, "dt_xdeepfm_infer_tower: flags 0x%x", flags);
    DT_REQUIRE(B == 0 || x0_out, "dt_xdeepfm_infer_tower: x0_out is null");
    return infer_run("dt_xdeepfm_infer_tower", idx, idx_kind, table, row_offset, vocab, dense, B, F, D, Nd, 0, workspace,
                     partial_out, nullptr, oob_count, flags, stream, kXdNets, x0_out);
}

extern "C" int dt_xdeepfm_infer_cin(int layer, const float* x0, const float* y_prev, const float* bias, int act, int B, int F,
                                    int D, int Nd, int n_layers, const int* layer_sizes, int direct, int cin_mode,
                                    const void* workspace, float* y, void* stream) {
    const char* who = "dt_xdeepfm_infer_cin";
    DeepFmDims dm; int lpr;
    XdLayout x;
    DT_UNSUPPORTED(!deepfm_dims(1, F, D, Nd, &dm, &lpr), "%s: unsupported shape F=%d D=%d Nd=%d", who, F, D, Nd);
    DT_UNSUPPORTED(!xd_layout(F, dm.CP, n_layers, layer_sizes, direct, cin_mode, &x), "%s: CIN of %d layers, mode %d, F=%d", who,
                   n_layers, cin_mode, F);
    DT_REQUIRE(layer >= 0 && layer < x.n && B >= 0, "%s: layer %d of %d, B=%d", who, layer, x.n, B);
    if (B == 0) return DT_OK;
    DT_REQUIRE(x0 && y && workspace && (layer == 0 || y_prev), "%s: null pointer", who);
    // layer 0 crosses x0 with itself; layer k the leading Hk channels of layer k - 1's output, a view of its [B][L][D] rows
    const float* xk = layer ? y_prev : x0;
    const int64_t xk_bs = layer ? (int64_t)x.L[layer - 1] * D : (int64_t)F * D;
    return dt_cin_layer_fwd_packed(cin_mode, x0, xk, reinterpret_cast<const char*>(workspace) + x.filt[layer], bias, act, B, F,
                                   x.Hk[layer], x.L[layer], D, (int64_t)F * D, xk_bs, y, stream);
}

extern "C" int dt_xdeepfm_infer_head(const float* const* y, const float* partial, int B, int F, int D, int Nd, int n_layers,
                                     const int* layer_sizes, int direct, int cin_mode, const void* workspace, float* logit_out,
                                     float* out, int flags, void* stream) {
    const char* who = "dt_xdeepfm_infer_head";
    DeepFmDims dm; int lpr;
    XdLayout x;
    DT_UNSUPPORTED(!deepfm_dims(1, F, D, Nd, &dm, &lpr), "%s: unsupported shape F=%d D=%d Nd=%d", who, F, D, Nd);
    DT_UNSUPPORTED(!xd_layout(F, dm.CP, n_layers, layer_sizes, direct, cin_mode, &x), "%s: CIN of %d layers, mode %d, F=%d", who,
                   n_layers, cin_mode, F);
    DT_REQUIRE(B >= 0 && (flags & ~DT_INFER_SIGMOID) == 0, "%s: B=%d flags 0x%x", who, B, flags);
    if (B == 0) return DT_OK;
    DT_REQUIRE(y && partial && workspace && logit_out, "%s: null pointer", who);
    const float* ws = reinterpret_cast<const float*>(workspace);
    XdHeadArgs a{};
    for (int k = 0; k < x.n; ++k) {
        DT_REQUIRE(y[k] && (uintptr_t)y[k] % 16 == 0, "%s: y[%d] null or not 16-byte aligned", who, k);
        a.y[k] = y[k]; a.L[k] = x.L[k]; a.lo[k] = x.lo[k]; a.woff[k] = x.woff[k];
    }
    a.n = x.n;
    a.wex = ws + x.wex;
    a.bex = a.wex + ((x.P + 3) & ~3);
    a.head = ws + infer_ws_layout(dm.CP, 0, kXdNets).head;
    a.partial = partial; a.logit = logit_out; a.out = out;
    a.sigmoid = (flags & DT_INFER_SIGMOID) ? 1 : 0;
    a.B = B; a.D = D;
    hipLaunchKernelGGL(k_xdeepfm_head, dim3(ceil_div(B, kXdHeadRows)), dim3(64 * kXdHeadRows), 0, as_stream(stream), a);
    return launch_status(who);
}
