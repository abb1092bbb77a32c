// uu3d_train_forward.inc -- one training-mode call (TrainCall), its up-front checks, the context both halves of the step share
// (TrainCtx) and the training-mode forward.  Included by uu3d_api.hip behind uu3d_train_state.inc.

namespace {

float droppath_rate(float dpr, int i, int depth) { return depth > 1 ? dpr * (float)i / (float)(depth - 1) : 0.f; }

// One training-mode call as the caller issued it: its buffers and draws, the Dropout rates and seed in force at its forward
// (uu3d_train_set_dropout may change them before a tape's backward) and its other options.  Both halves of the step read the call from here.
struct TrainCall {
    const float* params = nullptr; const float* kp2d = nullptr; const uint8_t* mask = nullptr; int B = 0;
    float dp_rates[3] = {0.f, 0.f, 0.f}; const float* dp_u = nullptr; const float* tm_u = nullptr; float tm_rate = 0.f;
    float drop_rate = 0.f, attn_drop_rate = 0.f; unsigned long long drop_seed = 0;
    bool bn_inference = false;          // generic_forward: OUTPUT_BN layers read the moving statistics
    float* const* attn_out = nullptr;   // generic_forward (return_attention=True): per temporal block, where its attention maps go
    float* full_out = nullptr; float* central_out = nullptr;       // NULL: the workspace's copies
    void* workspace = nullptr; size_t workspace_bytes = 0;
};

}  // namespace

static TrainCall train_call(const uu3d_model* m, const float* params, const float* kp2d, const uint8_t* mask, int32_t B, const float* dp_rates3,
                            const float* dp_u, const float* tm_u, float tm_rate, float* full_out, float* central_out, void* workspace, size_t workspace_bytes) {
    TrainCall k;
    k.params = params; k.kp2d = kp2d; k.mask = mask; k.B = B;
    if (dp_rates3) for (int i = 0; i < 3; ++i) k.dp_rates[i] = dp_rates3[i];
    k.dp_u = dp_u; k.tm_u = tm_u; k.tm_rate = tm_rate;
    k.drop_rate = m->ts->drop_rate; k.attn_drop_rate = m->ts->attn_drop_rate; k.drop_seed = m->ts->drop_seed;
    k.full_out = full_out; k.central_out = central_out; k.workspace = workspace; k.workspace_bytes = workspace_bytes;
    return k;
}

// A temporal / strided attention layer of L tokens takes the tiled exact-f32 pair of uu3d_attn_long.h (train_check bounds L): <= 128 tokens,
// the attention backward holds a sequence's tiles in registers (attn_bwd_mfma_kernel, 8 waves of 16 tokens); longer layers with head dim 48
// and without attention Dropout take the pair (up to ATTN_LONG_MAX_L = 416 tokens)
static bool train_long_attn(const uu3d_config& c, const TrainCall& k, int L) {
    return L > 128 && c.d_temporal == 48 * c.num_heads && !(k.attn_drop_rate > 0.f);
}

// The up-front checks of a call; backward: those of the backward pass too (LDS of the backward attention kernels, 96 tokens with
// ATTENTION_DROP_RATE > 0), so that a backward pass is never refused halfway through.
static int train_check(uu3d_model* m, const TrainCall& k, bool backward) {
    const uu3d_config& c = m->cfg;
    if ((c.has_strided_input != 0) != (k.mask != nullptr)) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "stride_mask must be given iff the model has strided input");
    // USE_REFINE: temporal blocks without the full-sequence head; the reference's train step reads a full output it does not have
    if (!c.full_output && c.temporal_depth > 0)
        return fail(m, UU3D_ERR_UNSUPPORTED, "training with USE_REFINE (temporal blocks without the full-sequence head) is not supported");
    // token counts of the temporal / strided attention layers: L[0] = N is the temporal stack's (when it exists) and strided block 1's
    std::vector<int> attn_L(m->L.begin(), m->L.begin() + c.num_strided);
    if (c.num_strided == 0 && c.temporal_depth > 0) attn_L.push_back(c.num_frames);
    // with Dropout on the attention weights the generic kernels keep P and dS of a head in LDS: 96 tokens
    for (const int L : attn_L) {
        if (backward && k.attn_drop_rate > 0.f && L > 96) return fail(m, UU3D_ERR_UNSUPPORTED, "the training step with ATTENTION_DROP_RATE > 0 supports at most 96 tokens");
        const bool pair = train_long_attn(c, k, L);
        if (pair && L > ATTN_LONG_MAX_L) return fail(m, UU3D_ERR_UNSUPPORTED, "the training step supports at most 416 tokens");
        if (!pair && L > 128) return fail(m, UU3D_ERR_UNSUPPORTED, "the training step supports at most 128 tokens");
    }
    // The generic attention kernels keep a head's K / V (backward: + Q, dO and the P / dS matrices) in LDS: checked HERE, before anything is
    // enqueued -- a launch refused in the middle of the backward pass would leave a half-run step behind (and, with several ranks, gradient
    // buckets already handed to the all-reduce).  Which layers take those kernels: launch_attn_generic (uu3d_launch.h).
    {
        auto lds = [](int L, int dh, bool bwd) { const size_t tile = (size_t)L * (dh + 4); return sizeof(float) * (bwd ? 4 * tile + 2 * (size_t)L * (L + 1) : 2 * tile); };
        const size_t cap = (size_t)160 * 1024;
        const int dhs = c.d_spatial / c.num_heads, dht = c.d_temporal / c.num_heads, Jk = c.num_keypoints;
        char msg[200];
        // spatial stack: generic kernels unless the fused stack runs (compiled dims, no Dropout); d_h = 4 packs max(1, 128 / J) heads per workgroup
        const int pack = dhs == 4 ? std::max(1, 128 / Jk) : 1;
        if (lds(Jk, dhs, backward) * pack > cap) {
            snprintf(msg, sizeof msg, "spatial attention over %d keypoints with head dim %d needs %zu bytes of LDS (> 160 KiB)", Jk, dhs, lds(Jk, dhs, backward) * pack);
            return fail(m, UU3D_ERR_UNSUPPORTED, msg);
        }
        const bool temporal_generic = m->generic || k.attn_drop_rate > 0.f;        // else: attn_f32 forward / MFMA backward (d_h = 48, <= 128 tokens)
        if (temporal_generic)
            for (const int L : attn_L)
                if (!train_long_attn(c, k, L) && lds(L, dht, backward && (dht != 48 || k.attn_drop_rate > 0.f)) > cap) {
                    snprintf(msg, sizeof msg, "temporal attention over %d tokens with head dim %d needs %zu bytes of LDS (> 160 KiB) in the %s pass: "
                             "fewer tokens or a smaller head dim", L, dht, lds(L, dht, true), backward ? "backward" : "forward");
                    return fail(m, UU3D_ERR_UNSUPPORTED, msg);
                }
    }
    if (((uintptr_t)k.workspace & 255) != 0) return fail(m, UU3D_ERR_WORKSPACE, "workspace must be 256-byte aligned");
    if (k.workspace_bytes < train_carve(m, k.B, nullptr).bytes) return fail(m, UU3D_ERR_WORKSPACE, "workspace smaller than uu3d_train_workspace_bytes(batch)");
    return UU3D_OK;
}

namespace {

// The shape of a transformer block: nseq sequences of L tokens (= rows per DropPath sample), width d, hidden width h; gelu: a spatial
// block (GELU MLP, H saved before it), else ReLU.  The two DropPath gates of a block: g1 the attention branch's, g2 the MLP branch's,
// nullptr = gate not drawn.
struct BlockShape { int nseq, L, d, h; bool gelu; int rows() const { return nseq * L; } };
struct Gates { const float* g1 = nullptr; const float* g2 = nullptr; float keep = 1.f; };

// What the forward and the backward half of a call derive from it alike: the carved workspace, the shapes, the weight table, the
// GEMM launcher on the operand arena, the Dropout sites, the DropPath gates (the gates themselves live in the workspace, written by
// the forward) and the attention kernel of each layer.  forward() and backward() are the two halves.
struct TrainCtx {
    uu3d_model* m; TrainState& t; const uu3d_config& c; const TrainCall& k; TrainWs w; hipStream_t stream;
    const NetW& nw;
    int B, N, J, ds, hs, dt, ht, Mt, Ms, J3, H, J3p, Ls, Lt, ns;
    bool h1;                                       // the full-sequence head (head1) exists
    float dpr_s, dpr_t, dpr_x;
    float* grads = nullptr;                        // backward(): the flat gradient buffer G() points into
    int st = UU3D_OK;
    Launcher Lh{m, stream, w.slab, kSlabFloats};
    TrainCtx(uu3d_model* m_, const TrainCall& k_, hipStream_t s)
        : m(m_), t(*m_->ts), c(m_->cfg), k(k_), w(train_carve(m_, k_.B, (char*)k_.workspace)), stream(s), nw(m_->ts->nw) {
        B = k.B; N = c.num_frames; J = c.num_keypoints; ds = c.d_spatial; hs = c.h_spatial; dt = c.d_temporal; ht = c.h_temporal;
        Mt = B * N; Ms = Mt * J; J3 = 3 * J; H = c.num_heads;
        J3p = round_up(J3, 32);                    // padded width of the head gradients = leading dimension of head1 / head2 .bwd
        Ls = c.spatial_depth; Lt = c.temporal_depth; ns = c.num_strided;
        h1 = has_head1(c);
        dpr_s = k.dp_rates[0]; dpr_t = k.dp_rates[1]; dpr_x = k.dp_rates[2];
    }
    // an offset of the weight table in the parameter / gradient buffer; -1 (the tensor does not exist) -> nullptr, here and nowhere else
    template <class T> static T* at(T* base, long long off) { return off < 0 ? nullptr : base + off; }
    const float* P(long long off) const { return at(k.params, off); }
    float* G(long long off) const { return at(grads, off); }
    const float* TA(size_t o) const { return t.tarena + o; }
    BlockShape shape_s() const { return BlockShape{Mt, J, ds, hs, true}; }
    BlockShape shape_t() const { return BlockShape{B, N, dt, ht, false}; }
    BlockShape shape_x(int j) const { return BlockShape{B, m->L[j], dt, ht, false}; }
    template <class AL, class EP>
    void gemm(const AL& al, const float* Bt, int M_, int N_, int K_, const EP& ep) {
        const _Float16* Bh = t.tarena_h ? t.tarena_h + (Bt - t.tarena) : nullptr;       // every Bt of the step lives in tarena
        const _Float16* Bl = t.tarena_h ? Bh + t.tarena_floats : nullptr;
        const int r = launch_gemm(al, Bt, M_, N_, K_, ep, w.slab, kSlabFloats, stream, Bh, Bl); if (r != UU3D_OK) st = r;
    }
    void first_error(int r) { if (r != UU3D_OK && st == UU3D_OK) st = r; }      // (status codes are values, not bits)
    static dim3 ew_grid(long long n) { return dim3((unsigned)((n + 255) / 256)); }
    // Dropout layers (uu3d_dropout.h): DROP_RATE at the projection / hidden / MLP-output / token_dropout sites, ATTENTION_DROP_RATE on the
    // attention weights.  Masks are a function of (seed, site, element): the backward pass recomputes them.
    // A block's first site: spatial 10 + 4 i, temporal 100 + 4 i, strided 200 + 4 j; + 0 attention weights, + 1 projection output,
    // + 2 hidden (ReLU blocks), + 3 MLP output
    DropCfg DR(unsigned site) const { return drop_cfg(k.drop_rate, k.drop_seed, site); }
    DropCfg AR(unsigned site) const { return drop_cfg(k.attn_drop_rate, k.drop_seed, site); }
    void drop_inplace(float* x, long long n, const DropCfg& d) const {
        if (d.on()) hipLaunchKernelGGL(dropout_inplace_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, n, d); }
    // DropPath gates (vision_transformer.py:16-43; rates linspace(0, dpr, depth), u_u_t.py:229-230,243-244) of block i of a stack: n
    // gate values per branch (one per DropPath sample)
    Gates gates(const float* base, float dpr, int i, int depth, size_t n) const {
        Gates g; g.keep = 1.f - droppath_rate(dpr, i, depth);
        if (k.dp_u && g.keep < 1.f) { g.g1 = base + (size_t)i * 2 * n; g.g2 = g.g1 + n; }
        return g;
    }
    Gates gates_s(int i) const { return gates(w.gates_s, dpr_s, i, Ls, Mt); }
    Gates gates_t(int i) const { return gates(w.gates_t, dpr_t, i, Lt, B); }
    Gates gates_x(int j) const { return gates(w.gates_x, dpr_x, j, ns, B); }
    // The attention kernels of a temporal / strided layer of L tokens, for both passes: the tiled exact-f32 pair (train_long_attn), else
    // the generic kernels with attention Dropout or generic dims, else the inference forward's attention; the backward of everything but
    // the pair is launch_attn_generic (uu3d_launch.h), which spatial layers take too.  ast: the pair's softmax row statistics in the
    // workspace (train_carve: layers of more than 128 tokens; nullptr: a spatial layer).  site: the layer's attention-Dropout site.
    bool long_attn(int L) const { return train_long_attn(c, k, L); }
    // the key mask of temporal block i / strided block j: without temporal blocks the first strided one must not attend to the upsampling
    // tokens (u_u_t.py:372-380; uu3d_create refuses FIRST_STRIDED_TOKEN_ATTENTION_LAYER > 1 there)
    const uint8_t* temporal_mask(int i) const { return (c.has_strided_input && i < c.first_strided_token_attention_layer) ? k.mask : nullptr; }
    const uint8_t* strided_mask(int j) const { return (Lt == 0 && c.has_strided_input && j < c.first_strided_token_attention_layer) ? k.mask : nullptr; }
    // head2's input x (rows ld apart): the last strided block's output, or without strided blocks the central token x[:, N // 2] of the
    // temporal stack's output (u_u_t.py:411-413) read in place, row N / 2 of every sequence (head2_row0 floats into the buffer)
    size_t head2_row0() const { return ns > 0 ? 0 : (size_t)(N / 2) * dt; }
    const float* head2_x() const { return (ns > 0 ? w.x_out : w.t_out) + head2_row0(); }
    int head2_ld() const { return ns > 0 ? dt : N * dt; }
    void attn_forward(const float* qkv, int L, const uint8_t* amask, float* O, float2* ast, unsigned site) {
        if (long_attn(L)) first_error(launch_attn_long(false, qkv, nullptr, nullptr, nullptr, 3 * dt, dt, B, L, H, amask, O, ast, dt, stream));
        else if (k.attn_drop_rate > 0.f || m->generic) first_error(launch_attn_generic(false, qkv, nullptr, 3 * dt, dt, B, L, H, dt / H, amask, O, dt, stream, AR(site)));
        else Lh.attn("train.attn", qkv, B, L, amask, O);
    }
    // dq | dk | dv of nseq sequences of L tokens and width d into dqkv, from O and dO
    void attn_backward(const float* qkv, const float* O, const float* dO, const float2* ast, int d, int nseq, int L, const uint8_t* amask,
                       float* dqkv, unsigned site) {
        if (ast != nullptr && long_attn(L)) first_error(launch_attn_long(true, qkv, O, dO, ast, 3 * d, d, nseq, L, H, amask, dqkv, nullptr, d, stream));
        else first_error(launch_attn_generic(true, qkv, dO, 3 * d, d, nseq, L, H, d / H, amask, dqkv, d, stream, AR(site), m->sw.train.attn_bwd_generic));
    }
    void droppath_gates();
    void block_forward(int L, const BlockAct& a, const BlockW& bw, const uint8_t* amask, float* maps, const Gates& g, unsigned site);
    int forward_begin();
    void forward_spatial();
    int forward_temporal();
    int forward();
    int forward_frames(const FramesIn& frames);
    int backward(float* grads, float gscale, const float* inv_scale_dev, float* grad_kp2d, bool ready, float* accum = nullptr);
};

}  // namespace

// The DropPath gates of the call, from its draws dp_u into the workspace: spatial blocks (2 Mt values each), temporal blocks (2 B each),
// strided blocks behind them (vision_transformer.py:16-43; rates linspace(0, dpr, depth), u_u_t.py:229-230,243-244)
void TrainCtx::droppath_gates() {
    if (k.dp_u == nullptr) return;                          // no gate is read (gates() returns nullptr)
    auto gate = [&](const float* u, float keep, int n, float* out) {
        hipLaunchKernelGGL(droppath_gate_kernel, ew_grid(n), dim3(256), 0, stream, keep < 1.f ? u : nullptr, n, keep, out); };
    const float* dp_u_t = k.dp_u + (size_t)Ls * 2 * Mt;
    if (Ls <= 16 && Lt <= 16) {                             // one launch for every layer of both stacks
        GateKeeps gk{};
        for (int i = 0; i < Ls; ++i) gk.s[i] = 1.f - droppath_rate(dpr_s, i, Ls);
        for (int i = 0; i < Lt; ++i) gk.t[i] = 1.f - droppath_rate(dpr_t, i, Lt);
        hipLaunchKernelGGL(droppath_gates_kernel, ew_grid((long long)Ls * 2 * Mt + (long long)Lt * 2 * B), dim3(256), 0, stream, k.dp_u, Ls, 2 * Mt, Lt, 2 * B, gk, w.gates_s, w.gates_t);
    } else {
        for (int i = 0; i < Ls; ++i) gate(k.dp_u + (size_t)i * 2 * Mt, 1.f - droppath_rate(dpr_s, i, Ls), 2 * Mt, w.gates_s + (size_t)i * 2 * Mt);
        for (int i = 0; i < Lt; ++i) gate(dp_u_t + (size_t)i * 2 * B, 1.f - droppath_rate(dpr_t, i, Lt), 2 * B, w.gates_t + (size_t)i * 2 * B);
    }
    // strided blocks (u_u_t.py:110,132-137; rates linspace(0, DROP_PATH_RATE[2], len(STRIDES)), :261-262): draws behind the temporal stack's
    if (dpr_x > 0.f) {
        const float* dp_u_x = dp_u_t + (size_t)Lt * 2 * B;
        for (int j = 0; j < ns; ++j) gate(dp_u_x + (size_t)j * 2 * B, 1.f - droppath_rate(dpr_x, j, ns), 2 * B, w.gates_x + (size_t)j * 2 * B);
    }
}

// A temporal / strided block of L tokens up to and including its inner Dropout: LayerNorm + q | k | v, attention, the projection with
// the DropPath-gated residual (g.g1), LayerNorm + fc1 + ReLU, the inner Dropout; the caller issues fc2 or the strided convolution.
// amask: the attention's token mask; maps: where the attention maps go (return_attention=True on a generic handle), else nullptr.
// site: the block's first Dropout site.
// LayerNorm-fed Dense layers (q | k | v, fc1): >= 1024 rows on the row-panel GEMM (ln_split_frag with the row statistics the
// backward pass reads + gemm_h3_panel_kernel), fewer rows / f32 training on the tiled kernel with the LayerNorm in its loader
void TrainCtx::block_forward(int L, const BlockAct& a, const BlockW& bw, const uint8_t* amask, float* maps, const Gates& g, unsigned site) {
    const int rows = B * L;
    const bool panel = t.pf_train != nullptr && rows >= 1024;
    if (panel) {
        Lh.ln_split_frag_stats("train.ln1", a.X, rows, P(bw.n1g), P(bw.n1b), w.Af, a.St1);
        Lh.gemm_panel_at("train.qkv", w.Af, t.pf_train + bw.pf_qkv, TA(bw.qkv.bias), rows, 3 * dt, PanelEpBias{a.QKV, 3 * dt});
    } else {
        launch_row_stats(a.X, dt, dt, rows, 1e-5f, a.St1, stream);
        gemm(ALoadLayerNorm{a.X, a.St1, P(bw.n1g), P(bw.n1b), dt, rows, dt}, TA(bw.qkv.fwd), rows, 3 * dt, dt, EpBias{a.QKV, TA(bw.qkv.bias), 3 * dt});
    }
    if (maps != nullptr)        // the maps recomputed from q | k (uu3d_misc.h), as the specialised path does
        hipLaunchKernelGGL(attn_probs_kernel, dim3(B * H), dim3(256), (size_t)L * (dt / H + 1) * sizeof(float), stream, (const void*)a.QKV, (const _Float16*)nullptr,
                           3 * dt, dt, L, H, dt / H, amask, 1.0f / sqrtf((float)(dt / H)), 0, maps);
    attn_forward(a.QKV, L, amask, a.O, a.Ast, site);
    gemm(ALoadPlain{a.O, dt, rows, dt}, TA(bw.proj.fwd), rows, dt, dt,
         EpBiasResGate{a.Xmid, a.X, P(bw.bp), dt, g.g1, g.keep, L, nullptr, nullptr, 1, DR(site + 1)});
    if (panel) {
        Lh.ln_split_frag_stats("train.ln2", a.Xmid, rows, P(bw.n2g), P(bw.n2b), w.Af, a.St2);
        Lh.gemm_panel_at("train.fc1", w.Af, t.pf_train + bw.pf_fc1, P(bw.b1), rows, ht, PanelEpBiasRelu{a.H, ht});
    } else {
        launch_row_stats(a.Xmid, dt, dt, rows, 1e-5f, a.St2, stream);
        gemm(ALoadLayerNorm{a.Xmid, a.St2, P(bw.n2g), P(bw.n2b), dt, rows, dt}, TA(bw.fc1.fwd), rows, ht, dt, EpBiasRelu{a.H, P(bw.b1), ht});
    }
    drop_inplace(a.H, (long long)rows * ht, DR(site + 2));        // inner dropout behind the ReLU (vision_transformer.py:63-64, u_u_t.py:84-85)
}

// The training-mode forward of a call, activations kept in the workspace: DropPath gates, the network, both heads -- everything up to
// where the loss starts.  Returns the status of its launches (hipGetLastError is the caller's).  Two stages: the spatial stage (the spatial
// stack, spatial_to_temporal_fc with the token blend and the temporal PE -> t_in) and everything from the temporal stack on
// (forward_temporal); the frames form of a generic handle (forward_frames) writes t_in from a feature table and runs the second stage alone.
int TrainCtx::forward() {
    const int r = forward_begin();
    if (r != UU3D_OK) return r;
    forward_spatial();
    return forward_temporal();
}

// uu3d_forward_frames_ex on a generic handle: t_in = (masked ? token : features[rows]) + temporal PE, then the second stage
int TrainCtx::forward_frames(const FramesIn& frames) {
    const int r = forward_begin();
    if (r != UU3D_OK) return r;
    hipLaunchKernelGGL(frames_to_tokens_kernel, ew_grid((long long)Mt * (dt / 4)), dim3(256), 0, stream, frames.features, frames.num_rows, frames.rows,
                       k.mask, P(nw.in_token), P(nw.pe_t), (long)Mt, N, dt, w.t_in);
    return forward_temporal();
}

int TrainCtx::forward_begin() {
    // The operand packs belong to whichever parameter buffer was repacked last.  On a generic-dims handle the model's inference forward (its own
    // buffer, uu3d_commit_weights) and a Trainer's step (its master buffer) alternate: a call whose `params` is not the packs' source
    // regenerates them first (ADVICE round 4: an EMA export left EMA-valued kernels under the trained biases of the next step).
    if (t.packed_from != k.params) {
        const int r = uu3d_train_repack(m, k.params, stream);
        if (r != UU3D_OK) return r;
    }
    m->prof_used = 0;
    droppath_gates();
    return UU3D_OK;
}

void TrainCtx::forward_spatial() {
    const bool dropping = k.drop_rate > 0.f || k.attn_drop_rate > 0.f;
    // =============================== forward (activations kept) ===============================
    if (t.sp_frag != nullptr && !dropping) {               // (the Dropout sites of the spatial stack exist in the unfused chain only)
        // the whole spatial stack in ONE launch (uu3d_spatial_h3.h, TRAIN = true): same arithmetic as the inference kernel, plus the
        // saved activations / row statistics the backward pass reads and the DropPath gates; 31 launches of the unfused chain
        SpatialParams sp{};
        sp.embed_w = P(nw.emb_w); sp.embed_b = P(nw.emb_b); sp.pe = P(nw.pe_s);
        sp.blocks = t.sp_blk; sp.norm_g = P(nw.sn_g); sp.norm_b = P(nw.sn_b);
        sp.depth = Ls; sp.total_frames = Mt; sp.frame_list = nullptr;
        SpatialTrainIO io{};
        for (int i = 0; i < Ls; ++i) {
            const BlockAct& a = w.sb[i];
            io.X[i] = a.X; io.St1[i] = a.St1; io.QKV[i] = a.QKV; io.O[i] = a.O; io.Xmid[i] = a.Xmid; io.St2[i] = a.St2; io.Hpre[i] = a.H;
            const Gates g = gates_s(i); io.gate1[i] = g.g1; io.gate2[i] = g.g2; io.inv_keep[i] = 1.0f / g.keep;
        }
        io.X[Ls] = w.s_out; io.StF = w.sStF;
        auto kern = spatial_stack_h3_kernel<kJ, kFR, 1, true>;
        hipLaunchKernelGGL(kern, dim3((Mt + kFR - 1) / kFR), dim3(128), sh3::lds_bytes(), stream, k.kp2d, sp, (const _Float16*)t.sp_frag, w.S,
                           (_Float16*)nullptr, (_Float16*)nullptr, io);
    } else {
        hipLaunchKernelGGL(embed_fwd_kernel, ew_grid((long long)Ms * ds), dim3(256), 0, stream, k.kp2d, P(nw.emb_w), P(nw.emb_b), P(nw.pe_s), Ms, J, ds, w.s_in);
        drop_inplace(w.s_in, (long long)Ms * ds, DR(1));                                   // token_dropout (u_u_t.py:324)
        for (int i = 0; i < Ls; ++i) {
            const BlockAct& a = w.sb[i]; const BlockW& bw = t.bw_s[i];
            const Gates g = gates_s(i);
            const unsigned site = 10u + 4u * (unsigned)i;
            launch_row_stats(a.X, ds, ds, Ms, 1e-5f, a.St1, stream);
            gemm(ALoadLayerNorm{a.X, a.St1, P(bw.n1g), P(bw.n1b), ds, Ms, ds}, TA(bw.qkv.fwd), Ms, 3 * ds, ds, EpBias{a.QKV, TA(bw.qkv.bias), 3 * ds});
            first_error(launch_attn_generic(false, a.QKV, nullptr, 3 * ds, ds, Mt, J, H, ds / H, nullptr, a.O, ds, stream, AR(site)));
            gemm(ALoadPlain{a.O, ds, Ms, ds}, TA(bw.proj.fwd), Ms, ds, ds,
                 EpBiasResGate{a.Xmid, a.X, P(bw.bp), ds, g.g1, g.keep, J, nullptr, nullptr, 1, DR(site + 1)});
            launch_row_stats(a.Xmid, ds, ds, Ms, 1e-5f, a.St2, stream);
            gemm(ALoadLayerNorm{a.Xmid, a.St2, P(bw.n2g), P(bw.n2b), ds, Ms, ds}, TA(bw.fc1.fwd), Ms, hs, ds, EpBias{a.H, P(bw.b1), hs});
            gemm(ALoadGelu{a.H, hs, Ms, hs}, TA(bw.fc2.fwd), Ms, ds, hs,
                 EpBiasResGate{a.Xout, a.Xmid, P(bw.b2), ds, g.g2, g.keep, J, nullptr, nullptr, 1, DR(site + 3)});
        }
        launch_row_stats(w.s_out, ds, ds, Ms, 1e-6f, w.sStF, stream);
        hipLaunchKernelGGL(ln_apply_kernel, ew_grid((long long)Ms * ds), dim3(256), 0, stream, w.s_out, w.sStF, P(nw.sn_g), P(nw.sn_b), Ms, ds, w.S);
    }
    // random token masking (u_u_t.py:287-311,336-338; masked-token value 0): rows that keep spatial_to_temporal_fc's output
    const uint8_t* keep_rows = nullptr;
    if (k.tm_u != nullptr && k.tm_rate > 0.f) {
        hipLaunchKernelGGL(token_keep_kernel, ew_grid(Mt), dim3(256), 0, stream, k.tm_u, k.tm_rate, k.mask, Mt, N, w.keep, w.keep + Mt);
        keep_rows = w.keep;
    }
    const float* mtoken = keep_rows != nullptr ? P(nw.mtoken) : nullptr;      // (nullptr without LEARNABLE_MASKED_TOKEN: value 0)
    gemm(ALoadPlain{w.S, J * ds, Mt, J * ds}, TA(nw.s2t.fwd), Mt, dt, J * ds,
         EpSpatialToTemporal{w.t_in, P(nw.s2t_b), dt, k.mask, P(nw.in_token), P(nw.pe_t), N, keep_rows, mtoken});
}

int TrainCtx::forward_temporal() {
    float* full = k.full_out ? k.full_out : w.full;
    float* central = k.central_out ? k.central_out : w.central;
    const float* pe_x0 = ns > 0 ? P(t.bw_x[0].pe) : nullptr;      // strided block 1 reads the temporal stack's output + its positional encoding
    for (int i = 0; i < Lt; ++i) {
        const BlockAct& a = w.tb[i]; const BlockW& bw = t.bw_t[i];
        const Gates g = gates_t(i);
        const bool last = (i + 1 == Lt) && ns > 0;         // strided block 1 reads t_out + its PE: the second store of the last fc2
        const unsigned site = 100u + 4u * (unsigned)i;
        block_forward(N, a, bw, temporal_mask(i), k.attn_out != nullptr ? k.attn_out[i] : nullptr, g, site);
        gemm(ALoadPlain{a.H, ht, Mt, ht}, TA(bw.fc2.fwd), Mt, dt, ht,
             EpBiasResGate{a.Xout, a.Xmid, P(bw.b2), dt, g.g2, g.keep, N, last ? w.x_in : nullptr, last ? pe_x0 : nullptr, N, DR(site + 3)});
    }
    // no temporal blocks: strided block 1 reads x + its PE (periodic over N), the second store the last fc2 would have made
    if (Lt == 0 && ns > 0)
        hipLaunchKernelGGL(add_period_kernel, ew_grid((long long)Mt * dt / 4), dim3(256), 0, stream, (const float*)w.t_in, pe_x0, Mt, dt, N, w.x_in);
    // OUTPUT_BN (u_u_t.py:275-285,400-404,414-416) in training mode: batch statistics of the head's input over every row, and the
    // moving statistics -- the last tensors of `params` -- updated in place as Keras does inside the training-mode call; x rows ldx apart
    const bool bn = c.output_bn != 0;
    auto MV = [&](long long off) { return const_cast<float*>(P(off)); };
    auto bn_forward = [&](const BnW& b, const float* x, int ldx, int rows, float* y, float* mean, float* rstd) {
        float* sum = w.bnv + 8 * dt; float* sq = w.bnv + 9 * dt;
        const long long n = (long long)rows * dt;
        if (k.bn_inference) {                            // generic_forward: the layer in inference mode (moving statistics, nothing written)
            hipLaunchKernelGGL(bn_moving_stats_kernel, ew_grid(dt), dim3(256), 0, stream, MV(b.mean), MV(b.var), 1e-5f, dt, mean, rstd);
            hipLaunchKernelGGL(bn_apply_kernel, ew_grid(n), dim3(256), 0, stream, x, mean, rstd, P(b.gamma), P(b.beta), n, dt, y, ldx);
            return;
        }
        int r = launch_colsum(x, ldx, rows, dt, 0, nullptr, 0, sum, 0, w.scratch, kOpScratchFloats, stream); if (r != UU3D_OK) st = r;
        hipLaunchKernelGGL(bn_sqdev_kernel, ew_grid(n), dim3(256), 0, stream, x, sum, 1.0f / (float)rows, n, dt, w.bnP, ldx);
        r = launch_colsum(w.bnP, dt, rows, dt, 0, nullptr, 0, sq, 0, w.scratch, kOpScratchFloats, stream); if (r != UU3D_OK) st = r;
        hipLaunchKernelGGL(bn_stats_kernel, ew_grid(dt), dim3(256), 0, stream, sum, sq, 1.0f / (float)rows, 1e-5f, 0.1f, dt, mean, rstd, MV(b.mean), MV(b.var));
        hipLaunchKernelGGL(bn_apply_kernel, ew_grid(n), dim3(256), 0, stream, x, mean, rstd, P(b.gamma), P(b.beta), n, dt, y, ldx);
    };
    if (h1) {
        const float* h1_in = w.t_out;
        if (bn) { bn_forward(nw.bn1, w.t_out, dt, Mt, w.bn1, w.bnv, w.bnv + dt); h1_in = w.bn1; }
        gemm(ALoadPlain{h1_in, dt, Mt, dt}, TA(nw.head1.fwd), Mt, J3, dt, EpBias{full, P(nw.h1_b), J3});
    }
    for (int j = 0; j < ns; ++j) {
        const BlockAct& a = w.xb[j]; const BlockW& bw = t.bw_x[j];
        const int Li = m->L[j], Lo = m->L[j + 1], Mo = B * Lo;
        const Gates g = gates_x(j);
        const unsigned site = 200u + 4u * (unsigned)j;
        block_forward(Li, a, bw, strided_mask(j), nullptr, g, site);
        const int lo = (c.strides[j] > 1 && c.pad_left[j] == 0) ? 1 : 0;
        gemm(ALoadConv3{a.H, ht, Li, Lo, c.strides[j], c.pad_left[j], Mo, 3 * ht}, TA(bw.fc2.fwd), Mo, dt, 3 * ht,
             EpConvResidual{a.Xout, P(bw.b2), dt, a.Xmid, Li, Lo, c.strides[j], lo, (j + 1 < ns) ? P(t.bw_x[j + 1].pe) : nullptr, g.g2, g.keep, DR(site + 3)});
    }
    const float* h2_in = head2_x(); int h2_ld = head2_ld();
    if (bn) { bn_forward(nw.bn2, h2_in, h2_ld, B, w.bn2, w.bnv + 2 * dt, w.bnv + 3 * dt); h2_in = w.bn2; h2_ld = dt; }
    gemm(ALoadPlain{h2_in, h2_ld, B, dt}, TA(nw.head2.fwd), B, J3, dt, EpBias{central, P(nw.h2_b), J3});
    if (Lh.status != UU3D_OK) st = Lh.status;
    return st;
}
