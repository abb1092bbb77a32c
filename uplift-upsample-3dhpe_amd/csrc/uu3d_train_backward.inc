// uu3d_train_backward.inc -- the backward pass of a training-mode call and the side streams its parameter-gradient work runs on.
// Included by uu3d_api.hip behind uu3d_train_forward.inc.

namespace {

// The stream choreography of one backward pass, over TrainState's side streams and events.  gemm_tn / colsum (parameter gradients)
// go to the side streams: a group() of them makes its side stream wait for what the main stream has produced so far; the main stream
// waits for side events only where it is about to overwrite something the side stream reads (see the marks in the backward pass).
struct SideStreams {
    static constexpr int kSide = TrainState::kSide;
    TrainState& t; const TrainWs& w; hipStream_t main;
    bool two = false;                                     // the side streams are in use (else: everything in order on the caller's stream)
    int cur = 0, fork_i = 0;                              // side stream of the current group of parameter-gradient launches; the next event of the ev_fork ring
    std::vector<std::function<void()>> ln_tail;           // combines of LayerNorm-backward partials waiting for the next group (see lnbwd)

    hipStream_t stream() const { return two ? t.side[cur] : main; }
    float* scratch() const { return two ? w.scratch2[cur] : w.scratch; }
    float* slab() const { return two ? w.slab2[cur] : w.slab; }
    // side stream s behind everything the main stream has enqueued so far (one event record + one stream wait)
    void fork(hipStream_t s) { hipEvent_t e = t.ev_fork[fork_i++ & 7]; (void)hipEventRecord(e, main); (void)hipStreamWaitEvent(s, e, 0); }
    // A step issued while the caller's stream is being captured into a hipGraph forks its side streams into the same capture
    // (event record / wait between capturing streams); UU3D_TRAIN_CAPTURE_INORDER=1 keeps a captured step on the caller's stream.
    void begin() {
        hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(main, &capturing);
        two = t.side[0] != nullptr && (capturing == hipStreamCaptureStatusNone || !process_switches().capture_inorder);
        if (two && capturing != hipStreamCaptureStatusNone) {   // every side stream joins the capture before anything records an event on it
            for (int k = 0; k < kSide; ++k) fork(t.side[k]);
            mark(t.ev_blk[0]); mark(t.ev_blk[1]);       // the first waits of the step would otherwise see the previous step's (uncaptured) records
        }
    }
    // group(fn): fn's launches (parameter gradients of one Dense layer / positional encoding) go to the next side stream, behind
    // everything the main stream has enqueued so far (one event record + one stream wait).  Queueing a block's groups and sending
    // them behind ONE record was measured after the buffer sets below went in and does not pay: 3.83 ms per step with a record
    // per group, 3.90 with two per block, 4.02 with one per block -- the later a group starts, the longer the tail.
    void group(const std::function<void()>& fn) {
        if (two) { cur = (cur + 1) % kSide; fork(t.side[cur]); }
        for (auto& tail : ln_tail) tail();
        ln_tail.clear();
        fn();
    }
    // a mark covers EVERY side stream (what one FIFO side stream implied: everything enqueued before the mark is done when it fires)
    void mark(hipEvent_t (&e)[kSide]) { if (two) for (int k = 0; k < kSide; ++k) (void)hipEventRecord(e[k], t.side[k]); }
    void wait(hipEvent_t (&e)[kSide]) { if (two) for (int k = 0; k < kSide; ++k) (void)hipStreamWaitEvent(main, e[k], 0); }
    void join_all() { if (!ln_tail.empty()) group([] {}); mark(t.ev_all); wait(t.ev_all); }
    // the stream on which a finished range of the gradient buffer is unscaled and handed on: side stream 0 behind the main stream and
    // behind every other side stream (a pending LayerNorm combine goes to a side stream first)
    hipStream_t gather() {
        if (!ln_tail.empty()) group([] {});
        if (!two) return main;
        hipStream_t s0 = t.side[0];
        fork(s0);
        for (int k = 1; k < kSide; ++k) { (void)hipEventRecord(t.ev_join[k], t.side[k]); (void)hipStreamWaitEvent(s0, t.ev_join[k], 0); }
        return s0;
    }
};

}  // namespace

// The backward pass of a call from the head gradients its caller left in the workspace (dFull / dCentral, multiplied by a power of two):
// every parameter gradient into `grads`, each finished range unscaled -- by 1 / gscale, or (inv_scale_dev != NULL) by the factor the
// cotangent pass left on the device -- and, with grad_kp2d, d / d kp2d.  accum != NULL (with inv_scale_dev): each finished range is
// unscaled into accum[range] += instead, and `grads` keeps the scaled values.  ready: finished ranges go to the grad-ready callback.
int TrainCtx::backward(float* grads_, float gscale, const float* inv_scale_dev, float* grad_kp2d, bool ready, float* accum) {
    grads = grads_;
    SideStreams ss{t, w, stream};
    ss.begin();
    const float inner_scale = k.drop_rate > 0.f ? 1.0f / (1.0f - k.drop_rate) : 1.f;
    const uint8_t* keep_rows = (k.tm_u != nullptr && k.tm_rate > 0.f) ? w.keep : nullptr;     // (written by the forward: token_keep_kernel)
    const float* mtoken = keep_rows != nullptr ? P(nw.mtoken) : nullptr;
    const bool bn = c.output_bn != 0;
    const float* h1_in = bn ? w.bn1 : w.t_out;
    const float* h2_in = bn ? w.bn2 : head2_x();
    const int h2_ld = bn ? dt : head2_ld();
    const bool tn_f16 = t.tarena_h != nullptr && !process_switches().tn_f32;        // (tn_f32: weight-gradient GEMMs back on the exact-f32 kernel)
    // parameter gradients, on the current side stream with its own slab / scratch; out == nullptr: the tensor does not exist
    auto gemm_tn_ep = [&](const auto& al, const float* Bm, int ldb, int R_, int P_, int Q_, const auto& ep) {
        const int r = launch_gemm_tn(al, Bm, ldb, R_, P_, Q_, ep, ss.slab(), kSlabFloats, ss.stream(), tn_f16); if (r != UU3D_OK) st = r; };
    auto gemm_tn = [&](const auto& al, const float* Bm, int ldb, int R_, int P_, int Q_, float* out, int ldo) {
        if (out) gemm_tn_ep(al, Bm, ldb, R_, P_, Q_, EpStore{out, ldo}); };
    auto colsum = [&](const float* x, int ldx, int R_, int C_, int period, const uint8_t* mk, int want, float* out) {
        if (!out) return;
        const int r = launch_colsum(x, ldx, R_, C_, period, mk, want, out, 0, ss.scratch(), kOpScratchFloats, ss.stream()); if (r != UU3D_OK) st = r; };
    // the gradients of a Dense layer's bias and kernel (weight-table offsets) as one group: dy = d(its output), rows x n, al its A operand
    auto dense_grads = [&](const auto& al, const float* dy, int rows, int kdim, int n, long long kernel, long long bias) {
        ss.group([&] { colsum(dy, n, rows, n, 0, nullptr, 0, G(bias)); gemm_tn(al, dy, n, rows, kdim, n, G(kernel), n); }); };
    // dx = res + d x (res == nullptr: d x alone) on the main stream; the combine of the partial dgamma / dbeta (in `part`) rides with
    // the next group of the side streams -- one launch less per LayerNorm on the activation-gradient chain
    // gated: the DropPath-gated copy of dx the next Dense-layer backward reads, written by the same kernel (no scale_rows launch)
    const LnBwdGated no_gate{nullptr, 1.f, 1, nullptr};
    auto lnbwd = [&](const float* x, const float* dy, const float2* stats, const float* gamma, int D_, int M_, float* dx, const float* res, float* dg, float* db, float* part,
                     const LnBwdGated& gated) {
        const int slices = launch_ln_bwd_rows(x, dy, stats, gamma, D_, D_, M_, dx, res != nullptr, res, part, kOpScratchFloats, stream, gated);
        ss.ln_tail.emplace_back([&ss, part, D_, slices, dg, db] { launch_ln_bwd_combine(part, D_, slices, dg, db, 0, ss.stream()); }); };
    auto scale_rows = [&](const float* in, int rows, int D_, const float* gate, float keep, int rps, const uint8_t* mk, int want, float* out) {
        hipLaunchKernelGGL(scale_rows_kernel, ew_grid((long long)rows * D_), dim3(256), 0, stream, in, rows, D_, gate, keep, rps, mk, want, out); };
    auto copy = [&](float* dst, const float* src, size_t n) { (void)hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToDevice, stream); };
    // [first, first + count) of the gradient buffer is final: unscaled (or unscaled into accum) and reported
    auto grads_done = [&](long long first, long long count) {
        if (count <= 0) return;
        hipStream_t s0 = ss.gather();
        if (accum != nullptr)
            hipLaunchKernelGGL(scale_accumulate_kernel, dim3((unsigned)std::min<long long>(4096, (count + 1023) / 1024)), dim3(256), 0, s0,
                               accum + first, (const float*)grads + first, count, inv_scale_dev, t.d_nonfinite);
        else if (inv_scale_dev != nullptr)
            hipLaunchKernelGGL(scale_flat_kernel, ew_grid(count), dim3(256), 0, s0, grads + first, count, 1.f, inv_scale_dev, t.d_nonfinite);
        else if (gscale != 1.f)
            hipLaunchKernelGGL(scale_flat_kernel, ew_grid(count), dim3(256), 0, s0, grads + first, count, 1.0f / gscale, (const float*)nullptr, t.d_nonfinite);
        if (ready && t.ready_fn) t.ready_fn(t.ready_user, (int64_t)first, (int64_t)count, (void*)s0);
    };

    // =============================== backward ===============================
    // Block k of the backward pass (strided, temporal and spatial blocks, and spatial_to_temporal_fc counted as one) keeps what
    // the side streams read of it -- d(block output) gin, the DropPath-gated copies gY / gY2, gH, gMid (d of the block's middle
    // residual), gQKV -- in buffer set k & 1, and writes its d(block input) to gOut[k & 1] with the LayerNorm backward that adds
    // the residual gradient out of place.  The only wait of the main stream is therefore the one in front of that last kernel,
    // for the side streams to be past block k - 1 (which read gOut[k & 1] as ITS gin): they have a whole block of main-stream
    // work to get there.  (Round 2 began with one set and two waits per block on marks recorded a third of a block earlier,
    // which stalled the main stream for about a quarter of the step.)
    int bk = 0;
    float* gin = w.gOut[1];
    // head2: d(its input) into gin = d x_out; without strided blocks into row N / 2 of every sequence of gin = d t_out (rows N d_t apart),
    // the other rows zero (head1's gradient is added to all of them further down)
    float* g2x = gin + head2_row0();
    const int g2ld = head2_ld();
    if (ns == 0) (void)hipMemsetAsync(gin, 0, (size_t)Mt * dt * sizeof(float), stream);
    hipLaunchKernelGGL(pad_cols_kernel, ew_grid((long long)B * J3p), dim3(256), 0, stream, w.dCentral, B, J3, J3p, w.dC64);
    ss.group([&] {
        gemm_tn(TnLoadPlain{h2_in, h2_ld, B, dt}, w.dC64, J3p, B, dt, J3, G(nw.h2_w), J3);
        colsum(w.dC64, J3p, B, J3, 0, nullptr, 0, G(nw.h2_b)); });
    // BatchNorm backward on the MAIN stream (the activation-gradient chain needs d gamma / d beta): d beta = colsum(dy), d gamma =
    // colsum(dy * xhat), dx = gamma * rstd * (dy - d beta / R - xhat * d gamma / R); dgv / dbv: where the dx kernel reads the two sums
    // (x and dx rows ldx apart, as in the forward's bn_forward)
    auto bn_backward_sums = [&](const BnW& b, const float* dy, const float* x, int ldx, int rows, const float* mean, const float* rstd) {
        const long long n = (long long)rows * dt;
        int r = launch_colsum(dy, dt, rows, dt, 0, nullptr, 0, G(b.beta), 0, w.scratch, kOpScratchFloats, stream); if (r != UU3D_OK) st = r;
        hipLaunchKernelGGL(bn_bwd_prod_kernel, ew_grid(n), dim3(256), 0, stream, dy, x, mean, rstd, n, dt, w.bnP, ldx);
        r = launch_colsum(w.bnP, dt, rows, dt, 0, nullptr, 0, G(b.gamma), 0, w.scratch, kOpScratchFloats, stream); if (r != UU3D_OK) st = r;
    };
    auto bn_backward_dx = [&](const BnW& b, const float* dy, const float* x, int ldx, int rows, const float* mean, const float* rstd,
                              const float* dgv, const float* dbv, float* dx, int accumulate) {
        const long long n = (long long)rows * dt;
        hipLaunchKernelGGL(bn_bwd_dx_kernel, ew_grid(n), dim3(256), 0, stream, dy, x, mean, rstd, P(b.gamma), dgv, dbv, 1.0f / (float)rows, n, dt, accumulate, dx, ldx);
    };
    if (bn) {
        for (const long long moving : {nw.bn1.mean, nw.bn1.var, nw.bn2.mean, nw.bn2.var})
            if (float* g0 = G(moving)) (void)hipMemsetAsync(g0, 0, (size_t)dt * sizeof(float), stream);      // not trainable: their slots of the gradient buffer are zeros
        gemm(ALoadPlain{w.dC64, J3p, B, J3p}, TA(nw.head2.bwd), B, dt, J3p, EpStore{w.bnT2, dt});
        bn_backward_sums(nw.bn2, w.bnT2, head2_x(), g2ld, B, w.bnv + 2 * dt, w.bnv + 3 * dt);
        bn_backward_dx(nw.bn2, w.bnT2, head2_x(), g2ld, B, w.bnv + 2 * dt, w.bnv + 3 * dt, G(nw.bn2.gamma), G(nw.bn2.beta), g2x, 0);
    } else
        gemm(ALoadPlain{w.dC64, J3p, B, J3p}, TA(nw.head2.bwd), B, dt, J3p, EpStore{g2x, g2ld});

    // the end of block bk: every side-stream reader of its buffer set is enqueued (mark), the side streams are past block bk - 1
    // (wait), and gOut[bk & 1] = gmid + d LN-in becomes the next block's gin.  x, st1, gamma / beta (weight-table offsets): the
    // LayerNorm whose backward this is, over `rows` rows of width d, d(its output) in gLN
    // next (optional): the gates of the NEXT block -- its gated d(block output) (g2), gY of the next set, is written here too; rps: its rows per sample
    bool gy_ready = false;
    auto block_done = [&](const float* x, const float2* st1, long long gamma, long long beta, int d, int rows, const float* gmid, const Gates& next, int rps) {
        const int pb = bk & 1;
        ss.mark(t.ev_blk[pb]);
        ss.wait(t.ev_blk[pb ^ 1]);
        lnbwd(x, w.gLN, st1, P(gamma), d, rows, w.gOut[pb], gmid, G(gamma), G(beta), w.lnP[pb][1], next.g2 ? LnBwdGated{next.g2, next.keep, rps, w.gY[pb ^ 1]} : no_gate);
        gin = w.gOut[pb]; ++bk; gy_ready = (next.g2 != nullptr);
    };
    // The attention half of a block, from dy1 = d(attention branch) (gated, Dropout applied) to block_done: the projection's gradients and
    // backward, the attention backward (site: the block's first Dropout site), the q | k | v gradients and backward; next: block_done's
    auto attn_half = [&](const BlockShape& sh, const BlockAct& a, const BlockW& bw, const float* dy1, const uint8_t* amask, unsigned site, const Gates& next) {
        const int rows = sh.rows(), d = sh.d;
        float* gq = w.gQKV[bk & 1];
        dense_grads(TnLoadPlain{a.O, d, rows, d}, dy1, rows, d, d, bw.wp, bw.bp);
        gemm(ALoadPlain{dy1, d, rows, d}, TA(bw.proj.bwd), rows, d, d, EpStore{w.gO, d});
        attn_backward(a.QKV, a.O, w.gO, a.Ast, d, sh.nseq, sh.L, amask, gq, site);
        // ONE weight-gradient GEMM over the concatenated d q | k | v (its three d x d column blocks go to the three kernels' gradients,
        // EpStore3) and one column sum for the three biases: a third of the launches of three separate groups, the LayerNorm of the
        // A operand recomputed once -- this group was the longest of a block and the side streams are what the main stream's one
        // wait per block waits for
        ss.group([&] {
            float* bq = G(bw.bq); float* bk_ = G(bw.bk); float* bv = G(bw.bv);
            if (bq && bk_ && bv) {
                const int r = launch_colsum(gq, 3 * d, rows, 3 * d, 0, nullptr, 0, ReduceOut{bq, bk_, bv, d}, 0, ss.scratch(), kOpScratchFloats, ss.stream());
                if (r != UU3D_OK) st = r;
            }
            gemm_tn_ep(TnLoadLayerNorm{a.X, a.St1, P(bw.n1g), P(bw.n1b), d, rows, d}, gq, 3 * d, rows, d, 3 * d, EpStore3{G(bw.wq), G(bw.wk), G(bw.wv), d}); });
        gemm(ALoadPlain{gq, 3 * d, rows, 3 * d}, TA(bw.qkv.bwd), rows, d, 3 * d, EpStore{w.gLN, d});
        block_done(a.X, a.St1, bw.n1g, bw.n1b, d, rows, w.gMid[bk & 1], next, sh.L);
    };

    for (int j = ns - 1; j >= 0; --j) {
        const BlockShape sh = shape_x(j); const BlockAct& a = w.xb[j]; const BlockW& bw = t.bw_x[j];
        const int Li = sh.L, Lo = m->L[j + 1], Mi = B * Li, Mo = B * Lo, s = c.strides[j], p0 = c.pad_left[j];
        const int lo = (s > 1 && p0 == 0) ? 1 : 0;
        const unsigned site = 200u + 4u * (unsigned)j;
        float *gmid = w.gMid[bk & 1], *gh = w.gH[bk & 1];
        // gin = d(block output) (Mo x dt); gz = d(MLP branch) = its DropPath-gated copy (the identity branch takes gin itself)
        const Gates g = gates_x(j);
        const float* gz = gin;
        if (g.g2 || k.drop_rate > 0.f) { scale_rows(gin, Mo, dt, g.g2, g.keep, Lo, nullptr, 0, w.gY[bk & 1]); gz = w.gY[bk & 1]; }
        drop_inplace(w.gY[bk & 1], (long long)Mo * dt, DR(site + 3));          // d(convolution output) = mask * d(dropped output)
        dense_grads(TnLoadConv3{a.H, ht, Li, Lo, s, p0, Mo, 3 * ht}, gz, Mo, 3 * ht, dt, bw.w2, bw.b2);
        if (s > 1) hipLaunchKernelGGL(identity_bwd_kernel, ew_grid((long long)Mi * dt), dim3(256), 0, stream, gin, B, Li, Lo, s, lo, dt, gmid);
        else copy(gmid, gin, (size_t)Mi * dt);
        gemm(ALoadConvT{gz, dt, Li, Lo, s, p0, Mi, 3 * dt}, TA(bw.fc2.convT), Mi, ht, 3 * dt, EpReluMask{gh, a.H, ht, inner_scale});
        dense_grads(TnLoadLayerNorm{a.Xmid, a.St2, P(bw.n2g), P(bw.n2b), dt, Mi, dt}, gh, Mi, dt, ht, bw.w1, bw.b1);
        gemm(ALoadPlain{gh, ht, Mi, ht}, TA(bw.fc1.bwd), Mi, dt, ht, EpStore{w.gLN, dt});
        lnbwd(a.Xmid, w.gLN, a.St2, P(bw.n2g), dt, Mi, gmid, gmid, G(bw.n2g), G(bw.n2b), w.lnP[bk & 1][0], no_gate);    // in place: no side-stream reader of gmid yet
        const float* dy1 = gmid;                                       // d(attention branch) = the DropPath-gated copy of d(mid stream)
        if (g.g1 || k.drop_rate > 0.f) { scale_rows(gmid, Mi, dt, g.g1, g.keep, Li, nullptr, 0, w.gY2[bk & 1]); dy1 = w.gY2[bk & 1]; }
        drop_inplace(w.gY2[bk & 1], (long long)Mi * dt, DR(site + 1));
        attn_half(sh, a, bw, dy1, strided_mask(j), site, Gates{});
        // (a reader of gOut that the NEXT block's mark covers)
        { float* go = gin; ss.group([&] { colsum(go, dt, Mi, dt, Li, nullptr, 0, G(bw.pe)); }); }
    }
    // head1: gin = d t_out (without temporal blocks there is no head1, and gin = d x_in = d t_in already)
    if (h1) {
        hipLaunchKernelGGL(pad_cols_kernel, ew_grid((long long)Mt * J3p), dim3(256), 0, stream, w.dFull, Mt, J3, J3p, w.dF64);
        ss.group([&] {
            gemm_tn(TnLoadPlain{h1_in, dt, Mt, dt}, w.dF64, J3p, Mt, dt, J3, G(nw.h1_w), J3);
            colsum(w.dF64, J3p, Mt, J3, 0, nullptr, 0, G(nw.h1_b)); });
        if (bn) {   // d(BN output) and the two sums before the tail of the gradient buffer is declared final; private copies of the sums for the dx
                    // kernel, which runs behind join_all -- by then grads_done's unscaling has rewritten the gradient slots
            gemm(ALoadPlain{w.dF64, J3p, Mt, J3p}, TA(nw.head1.bwd), Mt, dt, J3p, EpStore{w.bnT, dt});
            bn_backward_sums(nw.bn1, w.bnT, w.t_out, dt, Mt, w.bnv, w.bnv + dt);
            copy(w.bnv + 4 * dt, G(nw.bn1.gamma), (size_t)dt); copy(w.bnv + 5 * dt, G(nw.bn1.beta), (size_t)dt);
        }
    }
    // the tail of the buffer -- everything behind the temporal stack (or behind spatial_to_temporal_fc without one): strided blocks, the
    // heads and their BatchNorms -- is final (grads_done sends a pending LayerNorm combine to a side stream first)
    long long done_hi = t.n_params;
    grads_done(nw.tail_lo, done_hi - nw.tail_lo); done_hi = nw.tail_lo;
    ss.join_all();                               // the last strided block's PE column sum reads gin, which the next GEMM adds to
    if (h1) {
        if (bn) bn_backward_dx(nw.bn1, w.bnT, w.t_out, dt, Mt, w.bnv, w.bnv + dt, w.bnv + 4 * dt, w.bnv + 5 * dt, gin, 1);
        else gemm(ALoadPlain{w.dF64, J3p, Mt, J3p}, TA(nw.head1.bwd), Mt, dt, J3p, EpAdd{gin, dt});
    }

    // one pre-LN transformer block (temporal or spatial): gin = d X_out on entry, d X_in on exit.  g: the block's gates; next: those of
    // the next block of the backward pass; site: the block's first Dropout site
    auto block_backward = [&](const BlockShape& sh, const BlockAct& a, const BlockW& bw, const Gates& g, const uint8_t* amask, const Gates& next, unsigned site) {
        const int rows = sh.rows(), d = sh.d, h = sh.h, rps = sh.L;
        float *gmid = w.gMid[bk & 1], *gh = w.gH[bk & 1];
        const float* dy2 = gin;
        if (g.g2) { if (!gy_ready) scale_rows(gin, rows, d, g.g2, g.keep, rps, nullptr, 0, w.gY[bk & 1]); dy2 = w.gY[bk & 1]; }
        else if (k.drop_rate > 0.f) { scale_rows(gin, rows, d, nullptr, 1.f, rps, nullptr, 0, w.gY[bk & 1]); dy2 = w.gY[bk & 1]; }
        drop_inplace(w.gY[bk & 1], (long long)rows * d, DR(site + 3));                  // d(fc2 output) = mask * d(dropped output)
        gy_ready = false;
        if (sh.gelu) dense_grads(TnLoadGelu{a.H, h, rows, h}, dy2, rows, h, d, bw.w2, bw.b2);
        else dense_grads(TnLoadPlain{a.H, h, rows, h}, dy2, rows, h, d, bw.w2, bw.b2);
        if (sh.gelu) gemm(ALoadPlain{dy2, d, rows, d}, TA(bw.fc2.bwd), rows, h, d, EpGeluGrad{gh, a.H, h});
        else gemm(ALoadPlain{dy2, d, rows, d}, TA(bw.fc2.bwd), rows, h, d, EpReluMask{gh, a.H, h, inner_scale});
        dense_grads(TnLoadLayerNorm{a.Xmid, a.St2, P(bw.n2g), P(bw.n2b), d, rows, d}, gh, rows, d, h, bw.w1, bw.b1);
        gemm(ALoadPlain{gh, h, rows, h}, TA(bw.fc1.bwd), rows, d, h, EpStore{w.gLN, d});
        lnbwd(a.Xmid, w.gLN, a.St2, P(bw.n2g), d, rows, gmid, gin, G(bw.n2g), G(bw.n2b), w.lnP[bk & 1][0],
              g.g1 ? LnBwdGated{g.g1, g.keep, rps, w.gY2[bk & 1]} : no_gate);      // gmid = gin + d LN2-in, gY2 = its gated copy
        const float* dy1 = g.g1 ? w.gY2[bk & 1] : gmid;
        if (k.drop_rate > 0.f) {
            if (!g.g1) { scale_rows(gmid, rows, d, nullptr, 1.f, rps, nullptr, 0, w.gY2[bk & 1]); dy1 = w.gY2[bk & 1]; }
            drop_inplace(w.gY2[bk & 1], (long long)rows * d, DR(site + 1));
        }
        attn_half(sh, a, bw, dy1, amask, site, next);
    };

    for (int i = Lt - 1; i >= 0; --i) {
        block_backward(shape_t(), w.tb[i], t.bw_t[i], gates_t(i), temporal_mask(i), i > 0 ? gates_t(i - 1) : Gates{}, 100u + 4u * (unsigned)i);
        if (((Lt - 1 - i) & 1) == 1 || i == 0) {      // two temporal blocks (2 x 4.7 MB) per bucket
            const long long lo_ = t.bw_t[i].n1g;
            grads_done(lo_, done_hi - lo_); done_hi = lo_;
        }
    }
    // gin = d t_in : temporal PE, strided-input token, spatial_to_temporal_fc (a block of its own as far as the buffer sets go)
    ss.group([&] {
        colsum(gin, dt, Mt, dt, N, nullptr, 0, G(nw.pe_t));
        if (c.has_strided_input) colsum(gin, dt, Mt, dt, 0, k.mask, 0, G(nw.in_token));
        if (float* gm = G(nw.mtoken)) {          // (the weight exists: every gradient tensor is written every step)
            if (mtoken != nullptr) colsum(gin, dt, Mt, dt, 0, w.keep + Mt, 1, gm);
            else (void)hipMemsetAsync(gm, 0, (size_t)dt * sizeof(float), ss.stream());
        } });
    const float* dS2T = gin;
    if (c.has_strided_input || keep_rows != nullptr) {          // d s2t_out = d t_in on the rows that kept it (keep_rows folds the stride mask in)
        scale_rows(gin, Mt, dt, nullptr, 1.f, 1, keep_rows != nullptr ? keep_rows : k.mask, 1, w.gY[bk & 1]);
        dS2T = w.gY[bk & 1];
    }
    dense_grads(TnLoadPlain{w.S, J * ds, Mt, J * ds}, dS2T, Mt, J * ds, dt, nw.s2t_w, nw.s2t_b);
    gemm(ALoadPlain{dS2T, dt, Mt, dt}, TA(nw.s2t.bwd), Mt, J * ds, dt, EpStore{w.gLN, J * ds});
    // spatial_norm backward: (Mt x J*ds) viewed as (Ms x ds)
    block_done(w.s_out, w.sStF, nw.sn_g, nw.sn_b, ds, Ms, nullptr, Ls > 0 ? gates_s(Ls - 1) : Gates{}, J);
    for (int i = Ls - 1; i >= 0; --i)
        block_backward(shape_s(), w.sb[i], t.bw_s[i], gates_s(i), nullptr, i > 0 ? gates_s(i - 1) : Gates{}, 10u + 4u * (unsigned)i);
    // gin = d s_in: spatial PE, embedding (behind token_dropout: the same mask on the gradient)
    drop_inplace(gin, (long long)Ms * ds, DR(1));
    if (grad_kp2d != nullptr)                    // d kp2d = d s_in . W_emb^T, 0 on the rows the token blend discards
        hipLaunchKernelGGL(embed_input_grad_kernel, ew_grid(Ms), dim3(256), 0, stream, gin, P(nw.emb_w), Ms, J, ds,
                           keep_rows != nullptr ? keep_rows : k.mask, inv_scale_dev, grad_kp2d);
    ss.group([&] {
        colsum(gin, ds, Ms, ds, J, nullptr, 0, G(nw.pe_s));
        colsum(gin, ds, Ms, ds, 0, nullptr, 0, G(nw.emb_b)); });
    hipLaunchKernelGGL(embed_bwd_prep_kernel, ew_grid((long long)Ms * ds), dim3(256), 0, stream, k.kp2d, gin, Ms, ds, w.T);
    ss.group([&] { colsum(w.T, 2 * ds, Ms, 2 * ds, 0, nullptr, 0, G(nw.emb_w)); });
    grads_done(0, done_hi);                      // embedding, positional encodings, token, spatial stack, spatial_to_temporal_fc
    ss.join_all();                               // every gradient tensor is complete in stream order of the caller's stream

    hipError_t herr = hipGetLastError();
    if (herr == hipSuccess && st == UU3D_ERR_HIP) { herr = last_launch_error(); last_launch_error() = hipSuccess; }
    if (herr != hipSuccess && st == UU3D_OK) st = UU3D_ERR_HIP;
    if (st != UU3D_OK) return fail(m, st, std::string("training step launch failed") + (herr != hipSuccess ? std::string(": ") + hipGetErrorString(herr) : std::string()));
    return UU3D_OK;
}
