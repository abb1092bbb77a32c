// uu3d_train_entry.inc -- the entry points of the training step: the forward alone, the generic-dims forward, the step with the built-in
// loss, and the tape (a forward kept for a backward pass from caller-supplied output gradients).  Included last by uu3d_api.hip.

// What the entry points of the step begin with: uu3d_train_init has run, the handle's training lock is taken (`lock` holds it on return),
// no required buffer is NULL
static int train_enter(uu3d_model* m, std::unique_lock<std::recursive_mutex>& lock, bool buffers_ok) {
    if (!m->ts) return fail(m, UU3D_ERR_NOT_READY, "uu3d_train_init has not been called");
    lock = std::unique_lock<std::recursive_mutex>(m->train_mu);
    return buffers_ok ? UU3D_OK : fail(m, UU3D_ERR_INVALID_ARGUMENT, "null buffer");
}

// The training-mode forward of a call alone (model(inputs, training=True) without a tape, a tape's forward, generic_forward); backward:
// the backward pass's checks too
static int train_forward_only(uu3d_model* m, const TrainCall& k, bool backward, hipStream_t stream) {
    const int chk = train_check(m, k, backward);
    if (chk != UU3D_OK) return chk;
    HIPCHK(m, hipSetDevice(m->device));
    int st = TrainCtx(m, k, stream).forward();
    if (hipGetLastError() != hipSuccess && st == UU3D_OK) st = UU3D_ERR_HIP;
    return st == UU3D_OK ? UU3D_OK : fail(m, st, "training-mode forward launch failed");
}

// uu3d_forward_ex of a model with dims other than the compiled ones (uu3d_create): the training-mode forward chain with every stochastic
// layer off (no DropPath draws, no token mask, Dropout rates 0 for the call)
static int generic_forward(uu3d_model* m, const float* kp2d, const uint8_t* mask, int32_t B, float* full_out, float* central_out,
                           float* const* attn_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (m->ts == nullptr || m->gparams == nullptr) return fail(m, UU3D_ERR_NOT_READY, "uu3d_commit_weights has not been called");
    std::lock_guard<std::recursive_mutex> lock(m->train_mu);        // (the operand packs and their repack are the handle's)
    TrainCall k = train_call(m, m->gparams, kp2d, mask, B, nullptr, nullptr, nullptr, 0.f, full_out, central_out, workspace, workspace_bytes);
    k.drop_rate = 0.f; k.attn_drop_rate = 0.f; k.bn_inference = true; k.attn_out = attn_out;
    return train_forward_only(m, k, false, (hipStream_t)stream);
}

// uu3d_forward_frames_ex on a generic handle: the same call with its input tokens written from a feature table (TrainCtx::forward_frames);
// generic_forward's rules -- every stochastic layer off, OUTPUT_BN in inference mode, the training lock, the repack when the packs are not
// the handle's
static int generic_forward_frames(uu3d_model* m, const FramesIn& frames, const uint8_t* mask, int32_t B, float* full_out, float* central_out,
                                  float* const* attn_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (m->ts == nullptr || m->gparams == nullptr) return fail(m, UU3D_ERR_NOT_READY, "uu3d_commit_weights has not been called");
    std::lock_guard<std::recursive_mutex> lock(m->train_mu);
    TrainCall k = train_call(m, m->gparams, nullptr, mask, B, nullptr, nullptr, nullptr, 0.f, full_out, central_out, workspace, workspace_bytes);
    k.drop_rate = 0.f; k.attn_drop_rate = 0.f; k.bn_inference = true; k.attn_out = attn_out;
    const int chk = train_check(m, k, false);
    if (chk != UU3D_OK) return chk;
    HIPCHK(m, hipSetDevice(m->device));
    int st = TrainCtx(m, k, (hipStream_t)stream).forward_frames(frames);
    if (hipGetLastError() != hipSuccess && st == UU3D_OK) st = UU3D_ERR_HIP;
    return st == UU3D_OK ? UU3D_OK : fail(m, st, "uu3d_forward_frames_ex: launch failed");
}

// uu3d_frame_features on a generic handle: the spatial stack of every frame in one workgroup (uu3d_spatial_generic.h, reads the handle's
// master buffer) -> S (F, J d_s), then spatial_to_temporal_fc with its bias as the tiled GEMM on the handle's operand pack.  The workspace:
// S and the GEMM's split-K slab -- not the training workspace.
namespace {
struct GenericFrameWs { float *S, *slab; size_t bytes; };
GenericFrameWs generic_frame_carve(const uu3d_model* m, long F, char* base) {
    const size_t nS = align_up((size_t)F * m->cfg.num_keypoints * m->cfg.d_spatial * 4, 256);
    GenericFrameWs w{};
    w.bytes = nS + kSlabFloats * 4;
    if (base) { w.S = (float*)base; w.slab = (float*)(base + nS); }
    return w;
}
}  // namespace
static size_t generic_frame_features_bytes(const uu3d_model* m, long F) { return generic_frame_carve(m, F, nullptr).bytes; }

// The spatial launch of a generic handle, shared by generic_frame_features and the operator ABI (uu3d_op_spatial_stack): the repack when the
// packs are not the handle's, then spatial_generic_kernel, one workgroup per frame -> S (F, J d_s).  The training lock is held, the device set.
static int generic_spatial_launch(uu3d_model* m, const float* frames_dev, int32_t F, float* S, void* stream_, const char* who) {
    TrainState& t = *m->ts;
    const uu3d_config& c = m->cfg;
    if (t.packed_from != m->gparams) {
        const int r = uu3d_train_repack(m, m->gparams, stream_);
        if (r != UU3D_OK) return fail(m, r, std::string(who) + ": repack failed");
    }
    const int J = c.num_keypoints, ds = c.d_spatial;
    const NetW& nw = t.nw;
    SpatialGenericParams p{};
    p.params = m->gparams; p.blocks = t.d_sg_blocks;
    p.emb_w = nw.emb_w; p.emb_b = nw.emb_b; p.pe = nw.pe_s; p.norm_g = nw.sn_g; p.norm_b = nw.sn_b;
    p.J = J; p.ds = ds; p.hs = c.h_spatial; p.H = c.num_heads; p.depth = c.spatial_depth; p.hg = spatial_generic_head_group(J, c.num_heads);
    const size_t lds = spatial_generic_lds_bytes(J, ds, c.h_spatial, c.num_heads);      // (<= 160 KiB: has_frames_form, asked by the caller)
    allow_lds<spatial_generic_kernel<SG_ROWS>>(SG_LDS_LIMIT);
    hipLaunchKernelGGL(spatial_generic_kernel<SG_ROWS>, dim3((unsigned)F), dim3(SG_THREADS), lds, (hipStream_t)stream_, frames_dev, p, S);
    return UU3D_OK;
}

// uu3d_op_spatial_stack on a generic handle (arguments checked by the caller in uu3d_forward.inc)
static int generic_op_spatial_stack(uu3d_model* m, const float* frames_dev, int32_t F, float* S, void* stream_) {
    if (m->ts == nullptr || m->gparams == nullptr) return fail(m, UU3D_ERR_NOT_READY, "uu3d_commit_weights has not been called");
    std::lock_guard<std::recursive_mutex> lock(m->train_mu);
    HIPCHK(m, hipSetDevice(m->device));
    const int st = generic_spatial_launch(m, frames_dev, F, S, stream_, "uu3d_op_spatial_stack");
    if (st != UU3D_OK) return st;
    return hipGetLastError() == hipSuccess ? UU3D_OK : fail(m, UU3D_ERR_HIP, "uu3d_op_spatial_stack: launch failed");
}

static int generic_frame_features(uu3d_model* m, const float* frames_dev, int32_t F, float* features, void* workspace, size_t workspace_bytes,
                                  void* stream_) {
    if (m->ts == nullptr || m->gparams == nullptr) return fail(m, UU3D_ERR_NOT_READY, "uu3d_commit_weights has not been called");
    const GenericFrameWs w = generic_frame_carve(m, F, (char*)workspace);
    if (workspace_bytes < w.bytes) return fail(m, UU3D_ERR_WORKSPACE, "workspace smaller than uu3d_frame_features_bytes(frames)");
    std::lock_guard<std::recursive_mutex> lock(m->train_mu);        // (the s2t operand pack and its repack are the handle's)
    TrainState& t = *m->ts;
    const uu3d_config& c = m->cfg;
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(m, hipSetDevice(m->device));
    m->prof_used = 0;
    const int launched = generic_spatial_launch(m, frames_dev, F, w.S, stream_, "uu3d_frame_features");
    if (launched != UU3D_OK) return launched;
    const int J = c.num_keypoints, ds = c.d_spatial, dt = c.d_temporal;
    const NetW& nw = t.nw;
    const float* Bt = t.tarena + nw.s2t.fwd;
    const _Float16* Bh = t.tarena_h ? t.tarena_h + nw.s2t.fwd : nullptr;
    const _Float16* Bl = t.tarena_h ? Bh + t.tarena_floats : nullptr;
    int st = launch_gemm(ALoadPlain{w.S, J * ds, F, J * ds}, Bt, F, dt, J * ds, EpBias{features, m->gparams + nw.s2t_b, dt}, w.slab, kSlabFloats, stream, Bh, Bl);
    if (c.precision == UU3D_PREC_F16X3)           // range guard (include/uu3d.h): non-finite features set the model's sticky word
        hipLaunchKernelGGL(range_check_kernel, dim3(256), dim3(256), 0, stream, (const float*)features, (long)F * dt, (const float*)features, 0L, m->d_range);
    if (hipGetLastError() != hipSuccess && st == UU3D_OK) st = UU3D_ERR_HIP;
    return st == UU3D_OK ? UU3D_OK : fail(m, st, "uu3d_frame_features: launch failed");
}

int uu3d_train_forward_backward(uu3d_model* m, const float* params, const float* kp2d, const uint8_t* mask, const float* gt3d,
                                int32_t B, int32_t batch_size_norm, float w_center, float w_seq, int32_t root,
                                const float* dp_rates3, const float* dp_u, float* loss_out, float* full_out, float* central_out,
                                float* grads, void* workspace, size_t workspace_bytes, void* stream_) {
    return uu3d_train_forward_backward_masked(m, params, kp2d, mask, gt3d, B, batch_size_norm, w_center, w_seq, root, dp_rates3, dp_u,
                                              nullptr, 0.f, loss_out, full_out, central_out, grads, workspace, workspace_bytes, stream_);
}

int uu3d_train_forward_backward_masked(uu3d_model* m, const float* params, const float* kp2d, const uint8_t* mask, const float* gt3d,
                                       int32_t B, int32_t batch_size_norm, float w_center, float w_seq, int32_t root,
                                       const float* dp_rates3, const float* dp_u, const float* tm_u, float tm_rate,
                                       float* loss_out, float* full_out, float* central_out,
                                       float* grads, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    const bool fwd_only = (gt3d == nullptr);       // model(inputs, training=True) without a tape: training-mode forward only
    std::unique_lock<std::recursive_mutex> lock;
    const int ent = train_enter(m, lock, params && kp2d && workspace && B >= 1 && (fwd_only || (loss_out && grads)));
    if (ent != UU3D_OK) return ent;
    const TrainCall k = train_call(m, params, kp2d, mask, B, dp_rates3, dp_u, tm_u, tm_rate, full_out, central_out, workspace, workspace_bytes);
    hipStream_t stream = (hipStream_t)stream_;
    if (fwd_only) return train_forward_only(m, k, false, stream);
    const int chk = train_check(m, k, true);
    if (chk != UU3D_OK) return chk;
    HIPCHK(m, hipSetDevice(m->device));
    TrainCtx x(m, k, stream);
    const int st = x.forward();
    if (st != UU3D_OK) return fail(m, st, "training step launch failed");
    TrainState& t = *m->ts;
    const TrainWs& w = x.w;
    const int N = x.N, J = x.J;
    const float* full = x.h1 ? (full_out ? full_out : w.full) : nullptr;
    const float* central = central_out ? central_out : w.central;
    // =============================== loss ===============================
    // d loss / d pred is handed to the backward pass multiplied by a power of two `gscale`, and every finished range of the
    // gradient buffer is multiplied by 1 / gscale again (grads_done): with the production normaliser (BATCH_SIZE 512:
    // d loss / d joint = 0.5 / (512 * 71 * 17) = 8e-7) the unscaled back-propagated values sit below the smallest normal
    // half 6.1e-5, where the f16x3 split keeps them in the lo plane alone (11 bits) and flushes what is below 3e-8.
    // gscale puts the larger of the two loss-gradient magnitudes into (0.5, 1]; powers of two commute with every
    // rounding of the (linear) backward pass, so the exact-f32 kernels return bit-identical gradients either way.
    // Without the full-sequence head (no temporal blocks) the loss is (w_center + w_seq) * central (train.py:492-494): one term, whose
    // weight sets gscale alone.
    float gscale = 1.f;
    (void)hipMemsetAsync(t.d_nonfinite, 0, 16, stream);     // (every scale_flat launch is ordered behind the main stream from here on)
    {
        const float norm_cen = (float)batch_size_norm * (float)J, norm_seq = norm_cen * (float)N;
        const float w_cen = x.h1 ? w_center : w_center + w_seq;
        const float gmax = x.h1 ? fmaxf(fabsf(w_center) / norm_cen, fabsf(w_seq) / norm_seq) : fabsf(w_cen) / norm_cen;
        if (gmax > 0.f && t.tarena_h != nullptr) gscale = exp2f(-ceilf(log2f(gmax)));
        hipLaunchKernelGGL(mpjpe_loss_stage1, dim3(kLossGrid), dim3(256), 0, stream, full, central, gt3d, B, N, J, root,
                           gscale * (w_seq / norm_seq), gscale * (w_cen / norm_cen), x.h1 ? w.dFull : (float*)nullptr, w.dCentral, w.loss_scratch);
        hipLaunchKernelGGL(mpjpe_loss_stage2, dim3(1), dim3(64), 0, stream, w.loss_scratch, norm_seq, norm_cen, w_center, w_seq, x.h1 ? 1 : 0, loss_out);
    }
    return x.backward(grads, gscale, nullptr, nullptr, true);
}

// ---- the tape: a training-mode forward kept for a backward pass from caller-supplied output gradients (autograd) ----
struct uu3d_tape {
    TrainCall k;                 // the forward's buffers, draws and Dropout rates / seed
    float* own_grads = nullptr;  // parameter gradients of a backward pass called with grads_dev == NULL (allocated on first use)
    int device = 0;
};

int uu3d_train_forward_tape(uu3d_model* m, const float* params, const float* kp2d, const uint8_t* mask, int32_t B,
                            const float* dp_rates3, const float* dp_u, const float* tm_u, float tm_rate,
                            float* full_out, float* central_out, void* workspace, size_t workspace_bytes, uu3d_tape** out_tape, void* stream_) {
    if (!m || !out_tape) return UU3D_ERR_INVALID_ARGUMENT;
    *out_tape = nullptr;
    std::unique_lock<std::recursive_mutex> lock;
    const int ent = train_enter(m, lock, params && kp2d && workspace && B >= 1);
    if (ent != UU3D_OK) return ent;
    const TrainCall k = train_call(m, params, kp2d, mask, B, dp_rates3, dp_u, tm_u, tm_rate, full_out, central_out, workspace, workspace_bytes);
    const int r = train_forward_only(m, k, true, (hipStream_t)stream_);      // the backward's checks too: a tape's backward is never refused
    if (r != UU3D_OK) return r;
    uu3d_tape* tp = new uu3d_tape();
    tp->k = k; tp->device = m->device;
    *out_tape = tp;
    return UU3D_OK;
}

// The first half of a tape's backward: operand packs of the tape's parameters, then dFull / dCentral seeded with the cotangents times
// a power of two computed on the device (no host synchronisation).  *words_out: the loss scratch of the tape's workspace (unused by a
// tape's backward), where words[2] is the inverse that the unscaling of every finished gradient range and d kp2d read.
static int tape_seed(uu3d_model* m, uu3d_tape* tp, const float* grad_full, const float* grad_central, hipStream_t stream, float** words_out) {
    const TrainCall& k = tp->k;
    TrainState& t = *m->ts;
    HIPCHK(m, hipSetDevice(m->device));
    // another call may have regenerated the operand packs from a different buffer since the forward (as in uu3d_train_forward_backward)
    if (t.packed_from != k.params) {
        const int r = uu3d_train_repack(m, k.params, (void*)stream);
        if (r != UU3D_OK) return r;
    }
    const TrainWs w = train_carve(m, k.B, (char*)k.workspace);
    const bool h1 = has_head1(m->cfg);      // no full-sequence head: no dFull (grad_full must be NULL)
    if (!h1 && grad_full != nullptr) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "grad_full given, but the model has no full-sequence head (TEMPORAL_TRANSFORMER_BLOCKS = 0)");
    const long long nf = h1 ? (long long)k.B * m->cfg.num_frames * 3 * m->cfg.num_keypoints : 0LL, nc = (long long)k.B * 3 * m->cfg.num_keypoints;
    float* words = w.loss_scratch;
    HIPCHK(m, hipMemsetAsync(words, 0, 16, stream));
    const long long na = (grad_full ? nf : 0) + (grad_central ? nc : 0);
    if (na > 0) {
        const dim3 grid((unsigned)std::min<long long>(1024, (na + 255) / 256));
        hipLaunchKernelGGL(cot_absmax_kernel, grid, dim3(256), 0, stream, grad_full, grad_full ? nf : 0LL, grad_central, grad_central ? nc : 0LL, (unsigned*)words);
    }
    hipLaunchKernelGGL(cot_seed_kernel, dim3((unsigned)std::min<long long>(2048, (nf + nc + 255) / 256)), dim3(256), 0, stream, grad_full, nf, grad_central, nc,
                       w.dFull, w.dCentral, words, t.d_nonfinite);
    *words_out = words;
    return UU3D_OK;
}

int uu3d_train_backward_tape(uu3d_model* m, uu3d_tape* tp, const float* grad_full, const float* grad_central, float* grads,
                             float* grad_kp2d, void* stream_) {
    if (!m || !tp) return UU3D_ERR_INVALID_ARGUMENT;
    std::unique_lock<std::recursive_mutex> lock;
    const int ent = train_enter(m, lock, true);
    if (ent != UU3D_OK) return ent;
    HIPCHK(m, hipSetDevice(m->device));
    if (grads == nullptr) {
        if (tp->own_grads == nullptr) HIPCHK(m, hipMalloc((void**)&tp->own_grads, (size_t)m->ts->n_params * sizeof(float)));
        grads = tp->own_grads;
    }
    float* words = nullptr;
    const int r = tape_seed(m, tp, grad_full, grad_central, (hipStream_t)stream_, &words);
    if (r != UU3D_OK) return r;
    return TrainCtx(m, tp->k, (hipStream_t)stream_).backward(grads, 1.f, words + 2, grad_kp2d, false);
}

int uu3d_train_backward_tape_accumulate(uu3d_model* m, uu3d_tape* tp, const float* grad_full, const float* grad_central, float* grads_scratch,
                                        float* grads_accum, float* grad_kp2d, int32_t report_ranges, void* stream_) {
    if (!m || !tp) return UU3D_ERR_INVALID_ARGUMENT;
    if (!grads_scratch || !grads_accum) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "null gradient buffer");
    std::unique_lock<std::recursive_mutex> lock;
    const int ent = train_enter(m, lock, true);
    if (ent != UU3D_OK) return ent;
    const long long np_ = m->ts->n_params;                     // the unscale-and-add kernel reads one and writes the other (restrict)
    if (grads_scratch < grads_accum + np_ && grads_accum < grads_scratch + np_)
        return fail(m, UU3D_ERR_INVALID_ARGUMENT, "grads_scratch_dev and grads_accum_dev overlap");
    float* words = nullptr;
    const int r = tape_seed(m, tp, grad_full, grad_central, (hipStream_t)stream_, &words);
    if (r != UU3D_OK) return r;
    return TrainCtx(m, tp->k, (hipStream_t)stream_).backward(grads_scratch, 1.f, words + 2, grad_kp2d, report_ranges != 0, grads_accum);
}

void uu3d_tape_destroy(uu3d_tape* tp) {
    if (!tp) return;
    if (tp->own_grads) { (void)hipSetDevice(tp->device); (void)hipFree(tp->own_grads); }
    delete tp;
}
