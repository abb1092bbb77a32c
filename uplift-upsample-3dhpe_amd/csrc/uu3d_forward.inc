// uu3d_forward.inc -- workspace carving, the Launcher (one method per kind of launch) and the forward launch schedule: uu3d_forward*,
// uu3d_forward_frames_ex, uu3d_frame_features.  Included by uu3d_api.hip (one translation unit: the kernels are templates instantiated from here).

// ---- workspace --------------------------------------------------------------------------
namespace {
struct Workspace {
    float *S, *X, *QKV, *O, *Hb, *XA, *XB, *slab, *mslab;
    unsigned char* tc_scratch;     // temporal chain: the residual tiles between its launches (lane-linear), trash page (tchain16_scratch_bytes)
    int* frame_list;
    float2* stats;
    size_t slab_floats;
    size_t bytes;
};
Workspace carve(const uu3d_model* m, int B, char* base) {
    const uu3d_config& c = m->cfg;
    const size_t rows = (size_t)B * c.num_frames;
    const size_t rows_s = (size_t)B * (c.num_strided > 1 ? std::max(m->L[1], 1) : 1);
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off = align_up(off + n, 256); return o; };
    Workspace w{};
    const size_t oS = take(rows * c.num_keypoints * c.d_spatial * 4);
    const size_t oX = take(rows * c.d_temporal * 4);
    const size_t oQ = take((rows + 128) * 3 * c.d_temporal * 4);   // (+ one 128-row tile: the temporal chain writes q | k | v in whole tiles, fragment ordered)
    const size_t oO = take((rows + 32) * c.d_temporal * 4);   // + one 32-row panel: the panel GEMM's A operand is allocated in whole panels
    const size_t oH = take((rows + 32) * c.h_temporal * 4);   // + one 32-row panel (fragment-ordered hidden planes)
    const size_t oA = take(rows * c.d_temporal * 4);
    const size_t oB = take(rows_s * c.d_temporal * 4);
    const size_t oT = take(rows * sizeof(float2));
    w.slab_floats = (size_t)1536 * 4096;            // >= slices * M * N of any split GEMM (slices * tiles <= ~1150)
    const size_t oSl = take(w.slab_floats * 4);
    const size_t oFl = take((rows + 1) * sizeof(int));
    const size_t oMs = take((size_t)MLPF_SLICES * rows * c.d_temporal * 4);      // fused MLP: fc2 partial sums of the three hidden slices
    const size_t oCh = !tchain_possible(c) ? 0 : take(tchain16_scratch_bytes((int)((rows + 63) / 64)));
    w.bytes = off;
    if (base) {
        w.S = (float*)(base + oS); w.X = (float*)(base + oX); w.QKV = (float*)(base + oQ);
        w.O = (float*)(base + oO); w.Hb = (float*)(base + oH); w.XA = (float*)(base + oA);
        w.XB = (float*)(base + oB); w.stats = (float2*)(base + oT); w.slab = (float*)(base + oSl); w.frame_list = (int*)(base + oFl); w.mslab = (float*)(base + oMs);
        w.tc_scratch = !tchain_possible(c) ? nullptr : (unsigned char*)(base + oCh);
    }
    return w;
}
}  // namespace

size_t uu3d_workspace_bytes(const uu3d_model* m, int32_t batch) {
    if (!m || batch < 1) return 0;
    if (m->generic) return uu3d_train_workspace_bytes(m, batch);     // the generic forward keeps the training chain's activations
    return carve(m, batch, nullptr).bytes;
}

// ---- launch helpers ---------------------------------------------------------------------
namespace {

// Both spatial kernels work on 3 frames per workgroup and are latency bound: a launch takes (rounds of resident workgroups)
// x (one workgroup's run time).  Measured on MI355X, h36m_351 at batch 128 (3030 workgroups): the f16x3 kernel (two waves per
// workgroup, 26 KB LDS: 6 workgroups per CU = 1536 per round) 135 us for its two rounds; the exact-f32 kernel (one wave, 7 per
// CU = 1792 per round) ~133 us per round.  The frame count of the launch decides (an upper bound: masked frames drop out on
// the device).
inline bool spatial_h3_pays(int frames) {
    const int wgs = (frames + kFR - 1) / kFR;
    const int t_h3 = ((wgs + 1535) / 1536) * 68, t_f32 = ((wgs + 1791) / 1792) * 133;
    return t_h3 <= t_f32;
}

// UU3D_SKIP (uu3d_switches.h): the hooks exist only in TIMING BUILDS (-DUU3D_TIMING_BUILD: `python uplift-upsample-3dhpe_amd/build.py --timing`
// writes csrc/libuu3d_timing.so, whose uu3d_version() says so); the product library compiles them out: no environment variable can make it skip a launch.
#ifdef UU3D_TIMING_BUILD
inline int skip_mask() { return process_switches().skip; }
#else
inline constexpr int skip_mask() { return 0; }
#endif

struct Launcher {
    uu3d_model* m;
    hipStream_t stream;
    float* slab = nullptr;          // split-K partial sums
    size_t slab_floats = 0;
    bool throughput = false;        // this CALL's schedule (uu3d_forward_ex): launches shaped for CU-microseconds instead of latency
    int precision = UU3D_PREC_F16X3;   // this CALL's arithmetic: the handle's, or UU3D_PREC_F32 with UU3D_SCHEDULE_EXACT_F32
    int status = UU3D_OK;
    bool few_splits = false;        // this forward runs the temporal chain: its split-K GEMMs aim for splitk_target() workgroups

    void begin(const char* name, const char* kernel, double flops, double bytes) {
        if (!m->profiling) return;
        if (m->prof_used == m->prof.size()) {
            ProfRec r;
            if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) { status = UU3D_ERR_HIP; return; }
            m->prof.push_back(r);
        }
        ProfRec& r = m->prof[m->prof_used];
        r.name = name; r.kernel = kernel; r.flops = flops; r.bytes = bytes;
        (void)hipEventRecord(r.e0, stream);
    }
    void end() {
        if (m->profiling && m->prof_used < m->prof.size()) { (void)hipEventRecord(m->prof[m->prof_used].e1, stream); ++m->prof_used; }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess && status == UU3D_OK) { status = UU3D_ERR_HIP; m->err = std::string("kernel launch failed: ") + hipGetErrorString(e); }
    }

    // Workgroups a split-K GEMM aims for: enough to fill the chip three times over when the launch has it to itself (latency); under the throughput
    // schedule the chip is shared and a launch costs its CU-microseconds -- hundreds of workgroups that each wait ten microseconds for a few
    // hundred kilobytes are expensive then (round 5: strided blocks 2 and 3, 7 GFLOP, cost 9 % of the pipelined step)
    int splitk_target() const {
        // (h36m_351, batch 128, eight slots, ms per step by target: 768: 0.678, 384: 0.665, 192: 0.664, 96: 0.666, 48: 0.664 -- profiles/r05_tchain_ab.txt)
        return (throughput && few_splits) ? process_switches().thr_splitk_target : 768;      // (only beside the temporal chain: forwards without it stay bit-identical between the schedules)
    }
    // f16x3 GEMM whose A operand already is a pair of f16 planes (written by ln_split / attention / the ReLU
    // epilogue): LDS-DMA staged kernel, K % 32 == 0.  Same split-K policy as gemm().
    template <class GL, class EP>
    void gemm_g(const char* name, const GL& gl, const float* Bt, int M, int N, int K, const EP& ep, double extra_bytes = 0) {
        begin(name, "gemm_h3", 2.0 * M * (double)N * K, 4.0 * ((double)M * K + (double)N * K + (double)M * N) + extra_bytes);
        const auto it = m->hplanes.find((size_t)(Bt - m->arena));
        if ((K % 32) != 0 || it == m->hplanes.end()) { status = UU3D_ERR_INVALID_ARGUMENT; m->err = "gemm_g: operand without f16 planes or K % 32 != 0"; end(); return; }
        launch_fwd_gemm_g(stream, gl, m->harena + it->second.first, m->harena + it->second.second, M, N, K, ep, slab, slab_floats, splitk_target());      // tile shape and split: uu3d_launch.h
        end();
    }

    // Row-panel GEMM (uu3d_gemm_panel.h): C = A B + colv with A the fragment-ordered planes written by ln_split_frag and
    // B the fragment-ordered operand at harena + pf.  K = 384.  The split S of the N / 32 column chunks over workgroups
    // minimises rounds x (prologue + chunks per workgroup) for one workgroup per CU (measured order of the candidates
    // at M = 9088 / 4544, N = 1152 / 768: tools/gemm_panel_exp).
    static int panel_splits(int M, int N) {
        const int mt = (M + 127) / 128, chunks = N / 32;
        int best = 0; double best_cost = 1e30;
        for (int S = 1; S <= chunks; ++S) {
            if (chunks % S != 0 || chunks / S > PANEL_COLV_FLOATS / 32) continue;
            const int per_xcd = (mt * S + 7) / 8;                           // workgroups on the busiest XCD (32 CUs, one workgroup each)
            const double cost = (double)((per_xcd + 31) / 32) * (2.5 + (double)chunks / S);
            if (cost < best_cost) { best_cost = cost; best = S; }
        }
        return best;
    }
    bool panel_ok(int M, int N, int K, size_t pf) const {
        return !m->sw.no_panel && pf != 0 && K == 384 && N % 32 == 0 && M >= 1024 && (double)M * N * 4.0 < 4.0e9;      // 32-bit byte offsets in the epilogue stores
    }
    // The 8-wave form of the row-panel GEMM (uu3d_gemm_panel8.h: contraction split over wave pairs, two waves per SIMD) for the chunk
    // counts it is instantiated for; UU3D_PANEL4=1 keeps every launch on the 4-wave kernel (A/B measurements).  Returns false when
    // the caller has to launch the 4-wave kernel.
    static bool panel8_ok(int cpw) { return !process_switches().panel4 && panel8_has(cpw); }
    // the profile records' kernel name = the kernel SYMBOL's distinguishing part (bench.py picks the dominant kernel by it)
    template <class EP> static const char* panel_symbol(bool eight) {
        const char* e = std::is_same<EP, PanelEpBiasSplitQ>::value ? "BiasSplitQ" : std::is_same<EP, PanelEpBiasResidual>::value ? "BiasResidual"
                      : std::is_same<EP, PanelEpBiasResidualLn>::value ? "BiasResidualLn" : std::is_same<EP, PanelEpBiasReluSplit>::value ? "BiasReluSplit"
                      : std::is_same<EP, PanelEpBiasRelu>::value ? "BiasRelu" : "Bias";
        static thread_local char buf[32];
        std::snprintf(buf, sizeof buf, "%s<%s>", eight ? "gemm_panel8" : "gemm_panel", e);
        return buf;
    }
    // the launches themselves: uu3d_launch.h (shared with the operator ABI)
    template <class EP>
    bool launch_panel8(const _Float16* Af, const _Float16* Bf, const float* colv, int M, int mt, int S, int cpw, const EP& ep) {
        return panel8_ok(cpw) && uu3d::launch_panel8(stream, Af, Bf, colv, M, mt, S, cpw, ep);
    }
    template <class EP>
    void launch_panel4(const _Float16* Af, const _Float16* Bf, const float* colv, int M, int mt, int S, int cpw, const EP& ep) {
        uu3d::launch_panel4<EP>(stream, Af, Bf, colv, M, mt, S, cpw, ep);
    }
    // the operand given by address (training: the packs regenerated from the master buffer) -- K = 384, N % 32 == 0; S = 0: panel_splits
    template <class EP>
    void gemm_panel_at(const char* name, const _Float16* Af, const _Float16* Bf, const float* colv, int M, int N, const EP& ep, int S = 0) {
        const int K = 384, mt = (M + 127) / 128;
        if (S == 0) S = panel_splits(M, N);
        begin(name, panel_symbol<EP>(panel8_ok((N / 32) / S)), 2.0 * M * (double)N * K, 4.0 * ((double)M * K + (double)N * K + (double)M * N));
        if (!launch_panel8(Af, Bf, colv, M, mt, S, (N / 32) / S, ep)) launch_panel4(Af, Bf, colv, M, mt, S, (N / 32) / S, ep);
        end();
    }
    // the forward's: the operand at harena + pf; UU3D_PANEL_S forces the column ranges per row tile where they divide the chunks (A/B measurements)
    template <class EP>
    void gemm_panel(const char* name, const _Float16* Af, size_t pf, const float* colv, int M, int N, const EP& ep) {
        if (skip_mask() & 2) return;
        const int s = process_switches().panel_s;
        gemm_panel_at(name, Af, m->harena + pf, colv, M, N, ep, (s != 0 && (N / 32) % s == 0 && (N / 32) / s <= PANEL_COLV_FLOATS / 32) ? s : 0);
    }
    // x[M][384] += A B + colv in place (the attention projection on the residual stream): N = K = 384, the kernel's chunk loop unrolled
    // (CPW = 4 / 6 / 12 chunks per workgroup for 3 / 2 / 1 column ranges per row tile -- uu3d_gemm_panel.h says why)
    // ln_g / ln_b / ln_out (optional): LayerNorm 2 (eps 1e-5) of the finished rows as the next panel GEMM's A fragments, by the same launch
    // when it owns whole rows (throughput schedule, 8-wave kernel) -- returns true when it did, false when the caller still has to
    // launch ln_split_frag
    bool gemm_panel_residual(const char* name, const _Float16* Af, size_t pf, const float* colv, int M, float* x,
                             const float* ln_g = nullptr, const float* ln_b = nullptr, _Float16* ln_out = nullptr) {
        const int K = 384, N = 384, mt = (M + 127) / 128;
        if (skip_mask() & 4) return false;
        int S = 1; double best = 1e30;
        for (int s : {1, 2, 3}) {                                  // same cost model as panel_splits
            const int per_xcd = (mt * s + 7) / 8;
            const double cost = (double)((per_xcd + 31) / 32) * (2.5 + 12.0 / s);
            if (cost < best) { best = cost; S = s; }
        }
        // several forwards in flight: the fewest CU-microseconds win, not the shortest launch (h36m_351 batch 128, 9088 rows: S = 3 / 2 / 1
        // = 213 / 142 / 71 workgroups, 16.3 / 18.9 / 27.5 us per launch; one batch at a time 127.7 / 126.2 / 121.2 k sequences/s, four in
        // flight 167.3 / 169.2 / 171.3 k on the same box)
        // (... for launches that fill a good part of the chip.  With fewer than 64 row tiles -- strided block 2: 23 -- the launch holds few CUs either way, and what it
        // costs the pipelined step is its DURATION on its forward's queue: 34.6 us as 23 workgroups x 12 chunks with LayerNorm 2 inside against 12.2 + 7.2 us)
        if (throughput && mt >= 64) S = 1;
        if (process_switches().panel_proj_s != 0) S = process_switches().panel_proj_s;      // (A/B measurements)
        const bool ln_tail = S == 1 && ln_out != nullptr && !process_switches().no_ln_tail && panel8_ok(12);
        begin(name, ln_tail ? panel_symbol<PanelEpBiasResidualLn>(true) : panel_symbol<PanelEpBiasResidual>(panel8_ok(12 / S)),
              2.0 * M * (double)N * K, 4.0 * ((double)M * K + (double)N * K + 2.0 * (double)M * N));
        const PanelEpBiasResidual ep{x, N};
        if (ln_tail) {
            const PanelEpBiasResidualLn epl{{x, N}, ln_g, ln_b, 1e-5f, ln_out};
            if (launch_panel8(Af, m->harena + pf, colv, M, mt, 1, 12, epl)) { end(); return true; }
        }
        if (launch_panel8(Af, m->harena + pf, colv, M, mt, S, 12 / S, ep)) { end(); return false; }
        launch_panel4_residual(stream, Af, m->harena + pf, colv, M, mt, S, ep);
        end();
        return false;
    }
    void ln_split_frag_stats(const char* name, const float* x, int M, const float* g, const float* b, _Float16* Af, float2* stats) {
        begin(name, "ln_split_frag", 0.0, 8.0 * (double)M * 384);
        hipLaunchKernelGGL((ln_split_frag_stats_kernel<24, 8>), dim3((M + 7) / 8), dim3(128), 0, stream, x, 384, M, 1e-5f, g, b, Af, stats);
        end();
    }
    // LayerNorm (eps 1e-5) of M rows of 384 floats, written as the fragment-ordered planes of the panel GEMM's A operand
    void ln_split_frag(const char* name, const float* x, int M, const float* g, const float* b, _Float16* Af) {
        if (skip_mask() & 32) return;
        begin(name, "ln_split_frag", 0.0, 8.0 * (double)M * 384);
        hipLaunchKernelGGL((ln_split_frag_kernel<24, 8>), dim3((M + 7) / 8), dim3(128), 0, stream, x, 384, M, 1e-5f, g, b, Af);   // 8 rows per workgroup: 6.6 us at 9088 rows (16: 7.0, 32: 7.9, 4: 6.6)
        end();
    }

    // C[M][N] = A[M][K] * W on the tiled kernels: f16x3 (gemm_h3_kernel, the loader's rows split while they are staged) or exact f32
    // (gemm_f32_kernel) by this call's precision.  Tile shape, DEEP form and split: launch_fwd_gemm (uu3d_launch.h).
    template <class AL, class EP>
    void gemm(const char* name, const AL& al, const float* Bt, int M, int N, int K, const EP& ep, double extra_bytes = 0) {
        const bool h3 = (precision == UU3D_PREC_F16X3);
        begin(name, h3 ? "gemm_h3" : "gemm_f32", 2.0 * M * (double)N * K, 4.0 * ((double)M * K + (double)N * K + (double)M * N) + extra_bytes);
        const _Float16* Bh = nullptr; const _Float16* Bl = nullptr;
        if (h3) {
            const auto it = m->hplanes.find((size_t)(Bt - m->arena));
            if (it == m->hplanes.end()) { status = UU3D_ERR_INVALID_ARGUMENT; m->err = "operand without f16 planes"; end(); return; }
            Bh = m->harena + it->second.first; Bl = m->harena + it->second.second;
        }
        launch_fwd_gemm(stream, al, Bt, Bh, Bl, M, N, K, ep, slab, slab_floats, splitk_target(), precision);
        end();
    }

    // vit.MLP of a temporal block in one launch (uu3d_mlp_fused.h): partial fc2 sums of the 3 hidden slices -> mslab
    bool mlpf_ok(int M, const BlockDev& b) const {
        return !m->sw.no_mlpf && b.w2_mf != 0 && panel_ok(M, m->cfg.h_temporal, m->cfg.d_temporal, b.w1_pf);
    }
    void mlp_fused(const char* name, const _Float16* Af, const BlockDev& b, int M, float* mslab) {
        if (skip_mask() & 8) return;
        begin(name, "mlp_fused", 4.0 * M * (double)m->cfg.d_temporal * m->cfg.h_temporal, 4.0 * ((double)M * 384 + 2.0 * 384 * 768 + 3.0 * M * 384));
        launch_mlp_fused(stream, Af, m->harena + b.w1_pf, m->harena + b.w2_mf, b.b1, mslab, M);
        end();
    }
    // One launch of the temporal chain (uu3d_tchain16.h): the row-local stages of a block for every 64-row tile
    void tchain(const char* name, const uu3d_model::TcLaunch& t, int M, const _Float16* Of, float* X, float* XA, const float* pe, int period,
                _Float16* Q, _Float16* H, unsigned char* scratch) {
        if (skip_mask() & 128) return;
        const double cols = ((t.flags & TC_PROJ) ? 384.0 : 0.0) + ((t.flags & TC_MLP) ? 1536.0 : 0.0) + ((t.flags & TC_FC1_PLANES) ? 768.0 : 0.0) + ((t.flags & TC_QKV) ? 1152.0 : 0.0);
        begin(name, "tchain", 2.0 * M * 384.0 * cols, 4.0 * (384.0 * cols + 2.0 * M * 384.0 + ((t.flags & TC_QKV) ? M * 1152.0 : 0.0) + ((t.flags & TC_FC1_PLANES) ? M * 768.0 : 0.0)));
        if (!launch_tchain(stream, t.flags, M, m->harena + t.w_off, m->arena + t.p_off, attn_qscale(), Of, X, XA, pe, period, Q, H, scratch)) {
            status = UU3D_ERR_UNSUPPORTED; m->err = "temporal chain: unknown stage set";
        }
        end();
    }
    // the fused MLP's combine (x += b2 + slabs; optionally xa = x + pe) + LayerNorm + split into A fragments
    void ln_res_split_frag(const char* name, float* x, int M, const float* bias2, const float* mslab, float* xa, const float* pe, int period,
                           const float* g, const float* b, _Float16* Af) {
        if (skip_mask() & 64) return;
        begin(name, "ln_split_frag", 0.0, 4.0 * (double)M * 384 * (xa ? 8 : 7));
        hipLaunchKernelGGL((ln_res_split_frag_kernel<24, 8>), dim3((M + 7) / 8), dim3(128), 0, stream, x, 384, M, 1e-5f, bias2, mslab, xa, pe, period, g, b, Af);
        end();
    }

    // Few rows (strided blocks 2-3, the heads): one workgroup per 32 x 32 tile, split-K over its waves, LayerNorm in the loader
    // (uu3d_gemm_wt.h) -- one launch where the tiled path needs row_stats + split-K GEMM + splitk_reduce.
    bool wt_ok(const float* Bt, int K) const {
        return precision == UU3D_PREC_F16X3 && !m->sw.no_wt && (K % 16) == 0 && m->hplanes.count((size_t)(Bt - m->arena)) != 0;
    }
    template <class AL, class EP>
    void gemm_wt(const char* name, const AL& al, const float* Bt, int M, int N, int K, const EP& ep, double extra_bytes = 0) {
        const auto it = m->hplanes.find((size_t)(Bt - m->arena));
        const _Float16* Bh = m->harena + it->second.first; const _Float16* Bl = m->harena + it->second.second;
        begin(name, "gemm_wt", 2.0 * M * (double)N * K, 4.0 * ((double)M * K + (double)N * K + (double)M * N) + extra_bytes);
        if (!launch_gemm_wt(stream, al, Bh, Bl, M, N, K, ep)) { status = UU3D_ERR_UNSUPPORTED; m->err = "gemm_wt: contraction longer than 768"; }
        end();
    }

    void row_stats(const char* name, const float* x, int D, int M, float2* stats) {
        begin(name, "row_stats", 0.0, 4.0 * (double)M * D + 8.0 * M);
        hipLaunchKernelGGL(row_stats_kernel<4>, dim3((M + 3) / 4), dim3(256), 0, stream, x, D, D, M, 1e-5f, stats);
        end();
    }

    // which attention kernel a launch takes: attn_choose (uu3d_launch.h) on this call's precision and the handle's switches
    AttnRule attn_rule() const { AttnRule r; r.precision = precision; r.attn_f32 = m->sw.attn_f32; r.attn_wg = m->sw.attn_wg; return r; }
    bool attn_is_h3(int L, bool planes_out) const { return uu3d::attn_is_h3(attn_rule(), L, planes_out); }
    bool attn_h3_any(int L) const { return uu3d::attn_h3_any(attn_rule(), L); }
    float attn_qscale() const { return 1.44269504088896341f / sqrtf((float)kDH); }
    // split_lo_off != 0: the context rows go out as f16 planes (hi at out, lo split_lo_off halfs further)
    // frag: the context rows in the row-panel GEMM's A-fragment order instead of row-major planes (split_lo_off != 0 only)
    // qfrag: q | k | v arrive in the temporal chain's fragment order (uu3d_tchain16.h, tchain_qf_index) -- attn_h3_kernel only
    void attn(const char* name, const float* qkv, int B, int L, const uint8_t* mask, float* out, size_t split_lo_off = 0, bool frag = false, bool qfrag = false) {
        if (skip_mask() & 16) return;
        const int D = m->cfg.d_temporal, H = m->cfg.num_heads;
        const AttnRule rule = attn_rule();
        begin(name, attn_class_name(attn_choose(rule, L, H, split_lo_off != 0, qfrag)), 4.0 * B * (double)H * L * L * kDH, 4.0 * 4.0 * B * (double)L * D);
        if (launch_attn_infer(stream, qkv, D, B, L, H, mask, out, split_lo_off, frag, qfrag, rule) != UU3D_OK) {
            status = UU3D_ERR_UNSUPPORTED;
            m->err = qfrag ? "fragment-ordered q | k | v need attn_h3_kernel"
                           : "attention over more than 128 tokens needs the f16x3 path (precision f16x3, d_t and h_t multiples of 32) or, up to 416 tokens, a call under UU3D_SCHEDULE_EXACT_F32";
        }
        end();
    }
};

// Stages 1-2 for a list of M frames (the B * N frames of the window forward; the frame table of uu3d_frame_features):
//   compact_frames (mask given: the frames the stack has to compute) ; spatial_stack  kp2d -> S ; gemm  S x W_s2t -> ep
// Which spatial kernel runs, and whether it leaves S as the two f16 planes the LDS-DMA GEMM reads (no split in the GEMM's loader:
// 32.6 -> 29.6 us for the GEMM, the spatial kernel unchanged), is decided HERE and nowhere else.
// c: the call's configuration (precision: the handle's, or f32 under UU3D_SCHEDULE_EXACT_F32).  timing_skip: the launch honours UU3D_SKIP bit 1.
// The three launch helpers below are shared by spatial_stage and the operator ABI (uu3d_op_spatial_choice, uu3d_op_compact_frames,
// uu3d_op_spatial_stack at the end of this file): the rule, the grids, the LDS sizes and the arena pointers exist once.
enum SpatialKernel : int { SPATIAL_AUTO = 0, SPATIAL_F32 = 1, SPATIAL_H3_TILES = 2, SPATIAL_P16 = 3 };      // = UU3D_SPATIAL_* of include/uu3d_ops.h
struct SpatialChoice { int kernel; bool planes; };
inline const char* spatial_class_name(int kernel) { return kernel == SPATIAL_H3_TILES ? "spatial_h3" : kernel == SPATIAL_P16 ? "spatial_p16" : "spatial_mfma"; }
// c: the call's configuration (precision: the handle's, or f32 under UU3D_SCHEDULE_EXACT_F32); M: the frames of the launch
inline SpatialChoice spatial_choose(const uu3d_model* m, const uu3d_config& c, int M) {
    const bool h3 = c.precision == UU3D_PREC_F16X3 && !m->sw.spatial_f32 && (m->sw.spatial_h3_always || spatial_h3_pays(M));
    const bool planes = h3 && !m->sw.no_planes && (c.num_keypoints * c.d_spatial) % 32 == 0;
    return SpatialChoice{!h3 ? SPATIAL_F32 : m->sw.spatial_h3_tiles ? SPATIAL_H3_TILES : SPATIAL_P16, planes};
}
// mask[M] bytes -> list[M + 1]: the indices of the nonzero bytes in order, their count at list[M].  Launch only.
inline void launch_compact_frames(hipStream_t stream, const uint8_t* mask, int M, int* list) {
    hipLaunchKernelGGL(compact_frames_kernel, dim3(1), dim3(1024), 0, stream, mask, M, list);
}
// One spatial kernel (SPATIAL_F32 / _H3_TILES / _P16) over M frames on the handle's committed SpatialParams and fragment arenas.
// frame_list: launch_compact_frames' list, or nullptr for every frame.  s_lo != nullptr (f16x3 kernels): the result as f16 planes at s_hi / s_lo
// instead of f32 at S.  Launch only; the caller reads the launch error.
inline void launch_spatial_stack(const uu3d_model* m, hipStream_t stream, int kernel, const float* kp2d, int M, const int* frame_list, float* S, _Float16* s_hi, _Float16* s_lo) {
    SpatialParams sp = m->sp;
    sp.total_frames = M;
    sp.frame_list = frame_list;
    if (kernel == SPATIAL_H3_TILES)
        hipLaunchKernelGGL((spatial_stack_h3_kernel<kJ, kFR, kSpatialMT>), dim3((M + kFR - 1) / kFR), dim3(64 * (2 / kSpatialMT)), sh3::lds_bytes(), stream, kp2d, sp,
                           m->harena + m->sp_frag_off, S, s_hi, s_lo, SpatialTrainIO{});
    else if (kernel == SPATIAL_P16)
        hipLaunchKernelGGL((spatial_stack_p16_kernel<kJ, kP16FR, kP16PW>), dim3((M + kP16FR - 1) / kP16FR), dim3(64 * p16_waves(kJ, kP16FR, kP16PW)), sp16::lds_bytes<kP16FR>(m->cfg.spatial_depth),
                           stream, kp2d, sp, m->harena + m->sp_frag16_off, S, s_hi, s_lo);
    else
        hipLaunchKernelGGL((spatial_stack_mfma_kernel<kJ, kFR>), dim3((M + kFR - 1) / kFR), dim3(64), spatial_v2_lds_bytes(), stream, kp2d, sp, S);
}

template <class EP>
void spatial_stage(Launcher& Lh, const uu3d_config& c, const float* kp2d, int M, const uint8_t* mask, int* frame_list, float* S, bool timing_skip, const EP& ep) {
    uu3d_model* const m = Lh.m;
    const int J = c.num_keypoints, ds = c.d_spatial, dt = c.d_temporal;
    const SpatialChoice ch = spatial_choose(m, c, M);
    const bool planes = ch.planes;
    const bool skip = timing_skip && (skip_mask() & 1) && ch.kernel != SPATIAL_F32;
    if (mask != nullptr) {
        Lh.begin("compact_frames", "compact_frames", 0.0, (double)M * 5.0);
        launch_compact_frames(Lh.stream, mask, M, frame_list);
        Lh.end();
    }
    const double fl = (double)M * (2.0 * J * 2 * ds + c.spatial_depth * (4.0 * 2 * J * ds * ds + 8.0 * 4 * J * J * (ds / 8) + 2.0 * 2 * J * ds * kHS));
    _Float16* const s_hi = planes ? reinterpret_cast<_Float16*>(S) : (_Float16*)nullptr;
    _Float16* const s_lo = planes ? reinterpret_cast<_Float16*>(S) + (size_t)M * J * ds : (_Float16*)nullptr;
    Lh.begin("spatial_stack", spatial_class_name(ch.kernel), fl, 4.0 * M * J * (2.0 + ds));
    if (!skip) launch_spatial_stack(m, Lh.stream, ch.kernel, kp2d, M, mask != nullptr ? frame_list : nullptr, S, s_hi, s_lo);
    Lh.end();
    if (planes) Lh.gemm_g("s2t", GLoadPlain{s_hi, s_lo, J * ds, M}, m->s2t_wt, M, dt, J * ds, ep);
    else Lh.gemm("s2t", ALoadPlain{S, J * ds, M, J * ds}, m->s2t_wt, M, dt, J * ds, ep);
}

}  // namespace

int uu3d_forward(uu3d_model* m, const float* kp2d, const uint8_t* mask, int32_t B, float* full_out,
                 float* central_out, void* workspace, size_t workspace_bytes, void* stream_) {
    return uu3d_forward_attention(m, kp2d, mask, B, full_out, central_out, nullptr, workspace, workspace_bytes, stream_);
}

int uu3d_forward_attention(uu3d_model* m, const float* kp2d, const uint8_t* mask, int32_t B, float* full_out,
                           float* central_out, float* const* attn_out, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    return uu3d_forward_ex(m, kp2d, mask, B, full_out, central_out, attn_out, workspace, workspace_bytes,
                           m->throughput ? UU3D_SCHEDULE_THROUGHPUT : UU3D_SCHEDULE_LATENCY, stream_);
}

namespace {
// The input of uu3d_forward_frames_ex: the spatial stack's output per frame (uu3d_frame_features) and a table row per token.
struct FramesIn { const float* features; long num_rows; const int32_t* rows; };

constexpr int kFewRows = 512;                                 // up to here a LayerNorm-fed GEMM runs on gemm_h3_wt_kernel (measured: see DESIGN.md)

// One forward call: what every stage needs, and one method per stage.  forward_impl (below) calls them in launch order.
struct Forward {
    uu3d_model* const m;
    Launcher Lh;
    const Workspace w;
    const uu3d_config c;                                      // (a copy: UU3D_SCHEDULE_EXACT_F32 changes THIS call's arithmetic, not the handle's)
    const uint8_t* const mask;
    const int B;
    float* const full_out; float* const central_out; float* const* const attn_out;
    const bool part_body, part_tail;                          // timing builds (UU3D_TIMING_PARTS): only the launches up to the first strided block / only the ones behind it

    const int N = c.num_frames, J = c.num_keypoints, dt = c.d_temporal, ht = c.h_temporal, M = B * N;
    const bool has_h1 = c.full_output && c.temporal_depth > 0;
    // f16x3 with K % 32 == 0 everywhere: activations that feed a GEMM travel as f16 hi/lo planes (same bytes as the
    // f32 tensors they replace: O and Hb are reused) and the GEMMs are the LDS-DMA kernel gemm_h3g_kernel
    const bool planes = (c.precision == UU3D_PREC_F16X3) && (dt % 32 == 0) && (ht % 32 == 0) && !m->sw.no_planes;
    // Throughput schedule (several forwards share the chip): the TEMPORAL CHAIN (uu3d_tchain16.h) -- per block one attention launch and one
    // launch for everything row-local (projection + residual, LayerNorm 2, fc1, ReLU, fc2 + residual, the next block's LayerNorm 1 + QKV) by
    // workgroups that own 64 token rows: 2 T + 3 launches for T temporal blocks and the head of the first strided block instead of 5 T + 5,
    // no partial-sum slabs, no LayerNorm passes.
    const bool chain = Lh.throughput && planes && m->sw.tchain_mode != 0 && (m->sw.tchain_mode == 1 || (M + 127) / 128 >= m->sw.tchain_min_tiles) && !m->tchain.empty() && M >= 1024 &&
                       (Lh.attn_is_h3(N, true) || (m->sw.tchain_short && Lh.attn_h3_any(N))) && (c.num_strided == 0 || m->L[0] == N) && (double)M * 1152 * 4.0 < 4.0e9 &&
                       attn_out == nullptr;      // (return_attention=True: the maps kernel reads row-major q | k planes, the chain writes fragment order)
    _Float16* const Ph = reinterpret_cast<_Float16*>(w.O);    // LayerNorm output (fragment order), then attention output (planes)
    _Float16* const Hh = reinterpret_cast<_Float16*>(w.Hb);   // relu(fc1)
    const BlockDev* pend = nullptr;                           // the temporal block whose fused MLP left its fc2 partial sums in w.mslab (see block_head)
    float* xa = w.XA;                                         // the strided blocks' residual stream (after them: head2's input)
    char nm[48];

    // 1-2 from a feature table (uu3d_forward_frames_ex): the token blend and the temporal PE, nothing else
    void tokens_from_frames(const FramesIn& frames) {
        Lh.begin("frames_to_tokens", "frames_to_tokens", 0.0, 4.0 * 3.0 * M * dt);
        hipLaunchKernelGGL(frames_to_tokens_kernel, dim3((unsigned)(((size_t)M * (dt / 4) + 255) / 256)), dim3(256), 0, Lh.stream,
                           frames.features, frames.num_rows, frames.rows, mask, m->token, m->pe_t, (long)M, N, dt, w.X);
        Lh.end();
    }
    // 1. spatial stack, 2. spatial_to_temporal_fc + token blend + temporal PE
    void spatial(const float* kp2d) {
        spatial_stage(Lh, c, kp2d, M, mask, w.frame_list, w.S, true, EpSpatialToTemporal{w.X, m->s2t_b, dt, mask, m->token, m->pe_t, N});
    }

    // The first five launches of a transformer block (temporal: vit.py:176-188, strided: u_u_t.py:126-135), on the residual
    // stream x of Mr = B * L rows:  x += proj(MHA(LN1(x)));  Hb = relu(fc1(LN2(x)))  -- Hb as f16 planes when `planes`.
    //   LayerNorm-fed Dense layers: ln_split_frag + the row-panel GEMM (>= 1024 rows), else row_stats + the tiled GEMM
    //   with LayerNorm in its loader.
    // `prev` != nullptr: the previous temporal block ended in the fused MLP -- its fc2 result still sits in w.mslab; this
    // block's first LayerNorm launch adds it to the residual stream (for the first strided block: to w.X, and x = w.XA = X + pe).
    // `fuse_mlp`: stop after the second LayerNorm (its fragments in Ph feed mlp_fused).
    // returns the fragment-ordered LayerNorm-2 output when `fuse_mlp` stopped the block in front of the MLP (else nullptr)
    const _Float16* block_head(const char* tag, int i, const BlockDev& b, float* x, int L, const uint8_t* kmask, const BlockDev* prev, bool fuse_mlp) {
        const int Mr = B * L;
        auto name = [&](const char* what) { snprintf(nm, sizeof nm, "%s%d.%s", tag, i + 1, what); return nm; };
        _Float16* const Pl = Ph + (size_t)Mr * dt; _Float16* const Hl = Hh + (size_t)Mr * ht;
        // Few rows (strided block 3: 384): the LayerNorm-fed Dense layers as ONE launch each on gemm_h3_wt_kernel (LayerNorm in
        // the loader, split-K inside the workgroup) instead of row_stats + split-K GEMM + splitk_reduce.  Measured per layer
        // (h36m_351, batch 128, HIP events): 16.6 vs 14.2 + 6.3 us (QKV), 16.8 vs 12.7 + 6.4 us (fc1).  The other few-row GEMMs
        // (projection, strided convolution, heads) are SLOWER there -- 32 x 32 tiles re-read both operands too often
        // (conv: 29 vs 20 us, head1: 19 vs 12 us) -- and stay on the tiled kernels.
        // q / k / v for attn_h3_kernel: f16 planes (hi at QKV, lo Mr * 3 d_t halfs further), q pre-multiplied by log2(e) / sqrt(d_h)
        const bool qsplit = Lh.attn_is_h3(L, planes);
        _Float16* const Qh = reinterpret_cast<_Float16*>(w.QKV); _Float16* const Ql = Qh + (size_t)Mr * 3 * dt;
        const EpBiasSplitQ ep_qs{Qh, Ql, b.bqkv, 3 * dt, dt, Lh.attn_qscale()};
        const bool few = planes && Mr <= kFewRows && Lh.wt_ok(b.wqkv_t, dt) && Lh.wt_ok(b.w1_t, dt);
        auto maps = [&]() {
            if (attn_out != nullptr && tag[0] == 't' && attn_out[i] != nullptr) {        // return_attention=True: the block's attention maps, recomputed from q | k
                Lh.begin(name("attn_maps"), "attn_probs", 2.0 * B * (double)c.num_heads * L * L * kDH, 4.0 * B * (double)c.num_heads * L * L);
                const size_t lds = (size_t)L * (kDH + 1) * sizeof(float);
                allow_lds<attn_probs_kernel>(160 * 1024 - 256);
                if (qsplit) hipLaunchKernelGGL(attn_probs_kernel, dim3(B * c.num_heads), dim3(256), lds, Lh.stream, (const void*)Qh, (const _Float16*)Ql, 3 * dt, dt, L, c.num_heads, kDH, kmask, 1.0f, 1, attn_out[i]);
                else hipLaunchKernelGGL(attn_probs_kernel, dim3(B * c.num_heads), dim3(256), lds, Lh.stream, (const void*)w.QKV, (const _Float16*)nullptr, 3 * dt, dt, L, c.num_heads, kDH, kmask, 1.0f / sqrtf((float)kDH), 0, attn_out[i]);
                Lh.end();
            }
        };
        if (few) {
            WtLoadF32 l1{x, dt, Mr, dt, b.ln1_g, b.ln1_b, 1e-5f, 1};
            if (qsplit) Lh.gemm_wt(name("ln_qkv"), l1, b.wqkv_t, Mr, 3 * dt, dt, ep_qs);
            else Lh.gemm_wt(name("ln_qkv"), l1, b.wqkv_t, Mr, 3 * dt, dt, EpBias{w.QKV, b.bqkv, 3 * dt});
            maps();
            Lh.attn(name("attn"), w.QKV, B, L, kmask, w.O, (size_t)Mr * dt);
            { GLoadPlain gl{Ph, Pl, dt, Mr}; Lh.gemm_g(name("proj_res"), gl, b.wp_t, Mr, dt, dt, EpBiasResidual{x, b.bp, dt, nullptr, nullptr, 1}, 4.0 * Mr * dt); }
            WtLoadF32 l2{x, dt, Mr, dt, b.ln2_g, b.ln2_b, 1e-5f, 1};
            Lh.gemm_wt(name("ln_fc1"), l2, b.w1_t, Mr, ht, dt, EpBiasReluSplit{Hh, Hl, b.b1, ht});
            return nullptr;
        }
        if (prev != nullptr) {                                     // (same row count as the block that left it: the panel path holds)
            if (x == w.X) Lh.ln_res_split_frag(name("ln1_split"), w.X, Mr, prev->b2, w.mslab, nullptr, nullptr, 1, b.ln1_g, b.ln1_b, Ph);
            else Lh.ln_res_split_frag(name("ln1_split"), w.X, Mr, prev->b2, w.mslab, x, b.pe, L, b.ln1_g, b.ln1_b, Ph);
            if (qsplit) Lh.gemm_panel(name("ln_qkv"), Ph, b.wqkv_pf, b.bqkv, Mr, 3 * dt, PanelEpBiasSplitQ{Qh, Ql, 3 * dt, dt, Lh.attn_qscale()});
            else Lh.gemm_panel(name("ln_qkv"), Ph, b.wqkv_pf, b.bqkv, Mr, 3 * dt, PanelEpBias{w.QKV, 3 * dt});
        } else if (planes && Lh.panel_ok(Mr, 3 * dt, dt, b.wqkv_pf)) {
            Lh.ln_split_frag(name("ln1_split"), x, Mr, b.ln1_g, b.ln1_b, Ph);
            if (qsplit) Lh.gemm_panel(name("ln_qkv"), Ph, b.wqkv_pf, b.bqkv, Mr, 3 * dt, PanelEpBiasSplitQ{Qh, Ql, 3 * dt, dt, Lh.attn_qscale()});
            else Lh.gemm_panel(name("ln_qkv"), Ph, b.wqkv_pf, b.bqkv, Mr, 3 * dt, PanelEpBias{w.QKV, 3 * dt});
        } else {
            Lh.row_stats(name("stats1"), x, dt, Mr, w.stats);
            ALoadLayerNorm al{x, w.stats, b.ln1_g, b.ln1_b, dt, Mr, dt};
            if (qsplit) Lh.gemm(name("ln_qkv"), al, b.wqkv_t, Mr, 3 * dt, dt, ep_qs);
            else { EpBias ep{w.QKV, b.bqkv, 3 * dt}; Lh.gemm(name("ln_qkv"), al, b.wqkv_t, Mr, 3 * dt, dt, ep); }
        }
        maps();
        // projection on the row-panel GEMM (round 3): attn_h3_kernel writes the context rows in A-fragment order, the residual is
        // added in the epilogue from values requested a chunk earlier (UU3D_NO_PANEL_PROJ=1: the tiled LDS-DMA kernel)
        const bool pproj = planes && !m->sw.no_panel_proj && Lh.panel_ok(Mr, dt, dt, b.wp_pf);      // (every attention kernel writes either layout)
        Lh.attn(name("attn"), w.QKV, B, L, kmask, w.O, planes ? (size_t)Mr * dt : 0, pproj);
        const bool mlp_panel = planes && Lh.panel_ok(Mr, ht, dt, b.w1_pf);
        bool ln2_done = false;
        if (pproj) ln2_done = mlp_panel ? Lh.gemm_panel_residual(name("proj_res"), Ph, b.wp_pf, b.bp, Mr, x, b.ln2_g, b.ln2_b, Ph)
                                        : Lh.gemm_panel_residual(name("proj_res"), Ph, b.wp_pf, b.bp, Mr, x);
        else {
            EpBiasResidual ep{x, b.bp, dt, nullptr, nullptr, 1};
            if (planes) { GLoadPlain gl{Ph, Pl, dt, Mr}; Lh.gemm_g(name("proj_res"), gl, b.wp_t, Mr, dt, dt, ep, 4.0 * Mr * dt); }
            else { ALoadPlain al{w.O, dt, Mr, dt}; Lh.gemm(name("proj_res"), al, b.wp_t, Mr, dt, dt, ep, 4.0 * Mr * dt); }
        }
        if (mlp_panel) {
            if (!ln2_done) Lh.ln_split_frag(name("ln2_split"), x, Mr, b.ln2_g, b.ln2_b, Ph);      // (throughput schedule: LayerNorm 2 rode in the projection's launch)
            if (fuse_mlp) return Ph;
            Lh.gemm_panel(name("ln_fc1"), Ph, b.w1_pf, b.b1, Mr, ht, PanelEpBiasReluSplit{Hh, Hl, ht});
        } else {
            Lh.row_stats(name("stats2"), x, dt, Mr, w.stats);
            ALoadLayerNorm al{x, w.stats, b.ln2_g, b.ln2_b, dt, Mr, dt};
            if (planes) { EpBiasReluSplit ep{Hh, Hl, b.b1, ht}; Lh.gemm(name("ln_fc1"), al, b.w1_t, Mr, ht, dt, ep); }
            else { EpBiasRelu ep{w.Hb, b.b1, ht}; Lh.gemm(name("ln_fc1"), al, b.w1_t, Mr, ht, dt, ep); }
        }
        return nullptr;
    }

    // 3. temporal blocks as the temporal chain: launch 0 = LayerNorm 1 + QKV of block 1, then per block attention + one chain launch
    void temporal_chain() {
        _Float16* const Q = reinterpret_cast<_Float16*>(w.QKV);
        Lh.tchain("t1.ln_qkv", m->tchain[0], M, nullptr, w.X, nullptr, nullptr, 1, Q, nullptr, w.tc_scratch);
        for (int i = 0; i < c.temporal_depth; ++i) {
            const bool masked = c.has_strided_input && i < c.first_strided_token_attention_layer;
            snprintf(nm, sizeof nm, "t%d.attn", i + 1);
            Lh.attn(nm, w.QKV, B, N, masked ? mask : nullptr, w.O, (size_t)M * dt, true, true);
            const bool to_strided = i + 1 == c.temporal_depth && c.num_strided > 0;
            snprintf(nm, sizeof nm, "t%d.chain", i + 1);
            Lh.tchain(nm, m->tchain[i + 1], M, Ph, w.X, to_strided ? w.XA : nullptr, to_strided ? m->sblocks[0].pe : nullptr, N, Q, nullptr, w.tc_scratch);
        }
    }
    // 3. temporal blocks, one launch per stage: with >= 1024 token rows the MLP is one launch (uu3d_mlp_fused.h): its three partial fc2
    // sums are added to the residual stream by the NEXT block's first LayerNorm launch (`pend`).
    void temporal_blocks() {
        for (int i = 0; i < c.temporal_depth; ++i) {
            const BlockDev& b = m->tblocks[i];
            const bool masked = c.has_strided_input && i < c.first_strided_token_attention_layer;
            const bool last = (i + 1 == c.temporal_depth);
            // (the fused MLP leaves its result for the NEXT block's first LayerNorm launch: without strided blocks the last temporal block has none)
            const bool fuse = planes && Lh.mlpf_ok(M, b) && (last ? (c.num_strided > 0 && Lh.panel_ok(M, 3 * dt, dt, m->sblocks[0].wqkv_pf))
                                                                  : Lh.panel_ok(M, 3 * dt, dt, m->tblocks[i + 1].wqkv_pf));
            const _Float16* const a2 = block_head("t", i, b, w.X, N, masked ? mask : nullptr, pend, fuse);
            pend = nullptr;
            if (fuse) {
                snprintf(nm, sizeof nm, "t%d.mlp", i + 1);
                Lh.mlp_fused(nm, a2, b, M, w.mslab);
                pend = &b;
                continue;
            }
            const bool to_strided = last && c.num_strided > 0;
            EpBiasResidual ep_fc2{w.X, b.b2, dt, to_strided ? w.XA : nullptr, to_strided ? m->sblocks[0].pe : nullptr, N};
            snprintf(nm, sizeof nm, "t%d.fc2_res", i + 1);
            if (planes) { GLoadPlain gl{Hh, Hh + (size_t)M * ht, ht, M}; Lh.gemm_g(nm, gl, b.w2_t, M, dt, ht, ep_fc2, 4.0 * M * dt); }
            else { ALoadPlain al{w.Hb, ht, M, ht}; Lh.gemm(nm, al, b.w2_t, M, dt, ht, ep_fc2, 4.0 * M * dt); }
        }
    }
    // 4. head1: the full-sequence output from the temporal blocks' result
    void head1() {
        if (!has_h1) return;
        ALoadPlain al{w.X, dt, M, dt}; EpBias ep{full_out, m->h1_b, 3 * J};
        Lh.gemm("head1", al, m->h1_wt, M, 3 * J, dt, ep);
    }
    // 5. strided blocks (with head1 behind the first block's head)
    void strided_blocks() {
        float* xb = w.XB;
        const _Float16* const hzero = m->harena;                 // 64 zero halfs (uu3d_commit_weights)
        if (c.temporal_depth == 0 && c.num_strided > 0) {      // no temporal block whose epilogue adds the first strided PE (u_u_t.py:382-383)
            Lh.begin("s1.add_pe", "add_pe", 0.0, 12.0 * M * dt);
            hipLaunchKernelGGL(add_period_kernel, dim3((unsigned)(((size_t)M * dt / 4 + 255) / 256)), dim3(256), 0, Lh.stream, w.X, m->sblocks[0].pe, M, dt, N, w.XA);
            Lh.end();
        }
        for (int i = 0; i < c.num_strided; ++i) {
            const BlockDev& b = m->sblocks[i];
            const int Li = m->L[i], Lo = m->L[i + 1], Mi = B * Li, Mo = B * Lo;
            if (((skip_mask() & 256) || part_body) && i >= 1) continue;       // (timing experiments: the strided blocks behind the first / 512: the first)
            if (((skip_mask() & 512) || part_tail) && i == 0) { std::swap(xa, xb); xb = w.XA; continue; }
            // MaxPool1D(pool 1, stride s) on the trimmed sequence; stride 1 keeps x untrimmed (u_u_t.py:138-154)
            const int lo = (c.strides[i] > 1 && c.pad_left[i] == 0) ? 1 : 0;
            const EpConvResidual ep_conv{xb, b.b2, dt, xa, Li, Lo, c.strides[i], lo,
                                         (i + 1 < c.num_strided) ? m->sblocks[i + 1].pe : nullptr};
            // (without temporal blocks the first strided block is the one that must not attend to the upsampling tokens, u_u_t.py:372-376)
            const bool smask = c.temporal_depth == 0 && c.has_strided_input && i < c.first_strided_token_attention_layer;
            if (chain && i == 0) {
                // the chain's last launch left q | k | v of this block (LayerNorm 1 of xa = x + pe); its projection, LayerNorm 2 and fc1 are the next one
                Lh.attn("s1.attn", w.QKV, B, Li, nullptr, w.O, (size_t)Mi * dt, true, true);
                Lh.tchain("s1.chain", m->tchain[c.temporal_depth + 1], Mi, Ph, nullptr, xa, nullptr, 1, nullptr, Hh, w.tc_scratch);      // (its stream: xa, lane-linear in the scratch since the last temporal launch; row-major xa written here for the convolution's residual rows)
            } else
            block_head("s", i, b, xa, Li, smask ? mask : nullptr, i == 0 ? pend : nullptr, false);
            // head1 goes here: after strided block 1's first LayerNorm launch, which completes w.X when the last MLP was fused.  Nothing
            // downstream reads it, but a side stream next to the strided blocks measured SLOWER (1.085 vs 1.040 ms per forward
            // replayed from a hipGraph: the cross-stream edges cost more than the 12 us they hide).
            if (i == 0) head1();
            snprintf(nm, sizeof nm, "s%d.conv_res", i + 1);
            if (planes) { GLoadConv3 gl{Hh, Hh + (size_t)Mi * ht, hzero, ht, Li, Lo, c.strides[i], c.pad_left[i], Mo};
                          Lh.gemm_g(nm, gl, b.w2_t, Mo, dt, 3 * ht, ep_conv, 4.0 * Mo * dt); }
            else { ALoadConv3 al{w.Hb, ht, Li, Lo, c.strides[i], c.pad_left[i], Mo, 3 * ht};
                   Lh.gemm(nm, al, b.w2_t, Mo, dt, 3 * ht, ep_conv, 4.0 * Mo * dt); }
            std::swap(xa, xb);
            if (i == 0) xb = w.XA;   // XA (B*N rows) is free again; XB only needs B*L_1 rows
        }
    }
    // 6. head2: the central pose
    void head2() {
        // no strided blocks: the central token x[:, N // 2] (u_u_t.py:411-413) = row N / 2 of every sequence, leading dimension N d_t
        ALoadPlain al{c.num_strided > 0 ? xa : w.X + (size_t)(N / 2) * dt, c.num_strided > 0 ? dt : N * dt, B, dt};
        EpBias ep{central_out, m->h2_b, 3 * J};
        Lh.gemm("head2", al, m->h2_wt, B, 3 * J, dt, ep);
    }
    // range guard (include/uu3d.h): non-finite outputs of an f16x3 forward set the model's sticky word
    void range_check() {
        if (c.precision != UU3D_PREC_F16X3) return;
        Lh.begin("range_check", "range_check", 0.0, 4.0 * ((has_h1 ? (double)M * 3 * J : 0.0) + (double)B * 3 * J));
        hipLaunchKernelGGL(range_check_kernel, dim3(256), dim3(256), 0, Lh.stream, has_h1 ? full_out : central_out, has_h1 ? (long)M * 3 * J : 0L,
                           central_out, (long)B * 3 * J, m->d_range);
        Lh.end();
    }
};

// The forward of uu3d_forward_ex and uu3d_forward_frames_ex: stages 1-2 from the 2D windows (kp2d) or from a feature table (frames),
// everything from the temporal blocks on shared.  The launch order is DESIGN.md section 4.
int forward_impl(uu3d_model* m, const float* kp2d, const FramesIn* frames, const uint8_t* mask, int32_t B, float* full_out,
                 float* central_out, float* const* attn_out, void* workspace, size_t workspace_bytes, int32_t schedule, void* stream_) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    const bool exact_f32 = (schedule & UU3D_SCHEDULE_EXACT_F32) != 0;
    schedule &= ~UU3D_SCHEDULE_EXACT_F32;
    // TIMING EXPERIMENT (tools/tail_branch_exp.py; results wrong): 0x200 = only the launches up to the first strided block, 0x400 = only the ones behind it
    // (only with UU3D_TIMING_PARTS=1 in the environment: otherwise the bits are an invalid schedule like any other unknown value)
#ifdef UU3D_TIMING_BUILD
    const bool parts_ok = process_switches().timing_parts;
#else
    constexpr bool parts_ok = false;
#endif
    const bool part_body = parts_ok && (schedule & 0x200) != 0, part_tail = parts_ok && (schedule & 0x400) != 0;
    if (parts_ok) schedule &= ~0x600;
    if (schedule != UU3D_SCHEDULE_LATENCY && schedule != UU3D_SCHEDULE_THROUGHPUT) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "schedule must be UU3D_SCHEDULE_LATENCY or UU3D_SCHEDULE_THROUGHPUT");
    if (!m->committed) return fail(m, UU3D_ERR_NOT_READY, "uu3d_commit_weights has not been called");
    if ((!kp2d && !frames) || !central_out || !workspace || B < 1) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "null buffer or batch < 1");
    if (frames != nullptr) {
        if (!has_frames_form(m)) return no_frames_form(m, "uu3d_forward_frames_ex");
        if (!frames->features || !frames->rows || frames->num_rows < 1) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_forward_frames_ex: null features / rows or no feature rows");
        if (((uintptr_t)frames->features & 15) != 0 || (m->cfg.d_temporal % 4) != 0) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_forward_frames_ex: features must be 16-byte aligned");
    }
    uu3d_config c = m->cfg;                                // (a copy: UU3D_SCHEDULE_EXACT_F32 changes THIS call's arithmetic, not the handle's)
    if (exact_f32) {
        if (m->generic) return fail(m, UU3D_ERR_UNSUPPORTED, "UU3D_SCHEDULE_EXACT_F32: handles with generic dims have no exact-f32 forward");
        c.precision = UU3D_PREC_F32;
    }
    if ((c.has_strided_input != 0) != (mask != nullptr))
        return fail(m, UU3D_ERR_INVALID_ARGUMENT, "stride_mask must be given iff the model has strided input");
    if (c.full_output && c.temporal_depth > 0 && !full_out) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "full_out_dev is required for this model");
    if (((uintptr_t)workspace & 255) != 0) return fail(m, UU3D_ERR_WORKSPACE, "workspace must be 256-byte aligned");
    if (m->generic) {
        // dims other than the compiled ones: the training-mode chain, forward only, with every stochastic layer off (no DropPath draws, no token
        // mask, Dropout rates 0): vit / u_u_t in inference mode
        const int r = frames != nullptr ? generic_forward_frames(m, *frames, mask, B, full_out, central_out, attn_out, workspace, workspace_bytes, stream_)
                                        : generic_forward(m, kp2d, mask, B, full_out, central_out, attn_out, workspace, workspace_bytes, stream_);
        if (r == UU3D_OK && c.precision == UU3D_PREC_F16X3) {
            const bool has_full = c.full_output && c.temporal_depth > 0 && full_out != nullptr;
            hipLaunchKernelGGL(range_check_kernel, dim3(256), dim3(256), 0, (hipStream_t)stream_, has_full ? full_out : central_out,
                               has_full ? (long)B * c.num_frames * c.num_keypoints * 3 : 0L, central_out, (long)B * c.num_keypoints * 3, m->d_range);
        }
        return r;
    }
    const Workspace w = carve(m, B, (char*)workspace);
    if (workspace_bytes < w.bytes) return fail(m, UU3D_ERR_WORKSPACE, "workspace smaller than uu3d_workspace_bytes(batch)");
    if ((long)B * c.num_frames * c.num_keypoints > (1L << 30)) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "batch too large");

    HIPCHK(m, hipSetDevice(m->device));
    m->prof_used = 0;
    Forward f{m, Launcher{m, (hipStream_t)stream_, w.slab, w.slab_floats, schedule == UU3D_SCHEDULE_THROUGHPUT, c.precision}, w, c,
              mask, B, full_out, central_out, attn_out, part_body, part_tail};
    if (!part_tail) { if (frames != nullptr) f.tokens_from_frames(*frames); else f.spatial(kp2d); }
    f.Lh.few_splits = f.chain;                             // (from here on: the s2t GEMM above splits as it does without the chain)
    if (!part_tail) {
        if (f.chain) f.temporal_chain(); else f.temporal_blocks();
        if (c.num_strided == 0) f.head1();                 // (otherwise behind the head of strided block 1)
    }
    f.strided_blocks();
    if (!part_body) { f.head2(); f.range_check(); }
    return f.Lh.status;
}
}  // namespace


int uu3d_forward_ex(uu3d_model* m, const float* kp2d, const uint8_t* mask, int32_t B, float* full_out,
                    float* central_out, float* const* attn_out, void* workspace, size_t workspace_bytes, int32_t schedule, void* stream_) {
    return forward_impl(m, kp2d, nullptr, mask, B, full_out, central_out, attn_out, workspace, workspace_bytes, schedule, stream_);
}

int uu3d_forward_frames_ex(uu3d_model* m, const float* features, int64_t num_rows, const int32_t* rows, const uint8_t* mask, int32_t B,
                           float* full_out, float* central_out, float* const* attn_out, void* workspace, size_t workspace_bytes,
                           int32_t schedule, void* stream_) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    const FramesIn fin{features, (long)num_rows, rows};
    return forward_impl(m, nullptr, &fin, mask, B, full_out, central_out, attn_out, workspace, workspace_bytes, schedule, stream_);
}

// ---- per-frame features (spatial stack + spatial_to_temporal_fc, no blend, no PE) ---------------
namespace {
struct FrameWorkspace { float *S, *slab; size_t slab_floats, bytes; };
FrameWorkspace carve_frames(const uu3d_model* m, long F, char* base) {
    const uu3d_config& c = m->cfg;
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off = align_up(off + n, 256); return o; };
    FrameWorkspace w{};
    const size_t oS = take((size_t)F * c.num_keypoints * c.d_spatial * 4);
    w.slab_floats = (size_t)1536 * 4096;                           // split-K partial sums of the s2t GEMM (as carve())
    const size_t oSl = take(w.slab_floats * 4);
    w.bytes = off;
    if (base) { w.S = (float*)(base + oS); w.slab = (float*)(base + oSl); }
    return w;
}
}  // namespace

size_t uu3d_frame_features_bytes(const uu3d_model* m, int32_t frames) {
    if (!m || frames < 1 || !has_frames_form(m)) return 0;
    return m->generic ? generic_frame_features_bytes(m, frames) : carve_frames(m, frames, nullptr).bytes;
}

int uu3d_frame_features(uu3d_model* m, const float* frames_dev, int32_t F, float* features, void* workspace, size_t workspace_bytes,
                        int32_t schedule, void* stream_) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    const bool exact_f32 = (schedule & UU3D_SCHEDULE_EXACT_F32) != 0;
    schedule &= ~UU3D_SCHEDULE_EXACT_F32;
    if (schedule != UU3D_SCHEDULE_LATENCY && schedule != UU3D_SCHEDULE_THROUGHPUT) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "schedule must be UU3D_SCHEDULE_LATENCY or UU3D_SCHEDULE_THROUGHPUT");
    if (!has_frames_form(m)) return no_frames_form(m, "uu3d_frame_features");
    if (m->generic && exact_f32) return fail(m, UU3D_ERR_UNSUPPORTED, "UU3D_SCHEDULE_EXACT_F32: handles with generic dims have no exact-f32 forward");
    if (!m->committed) return fail(m, UU3D_ERR_NOT_READY, "uu3d_commit_weights has not been called");
    if (!frames_dev || !features || !workspace || F < 1) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "null buffer or frames < 1");
    if ((long)F * m->cfg.num_keypoints > (1L << 30)) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "too many frames");
    if (((uintptr_t)workspace & 255) != 0) return fail(m, UU3D_ERR_WORKSPACE, "workspace must be 256-byte aligned");
    if (m->generic) return generic_frame_features(m, frames_dev, F, features, workspace, workspace_bytes, stream_);
    const FrameWorkspace w = carve_frames(m, F, (char*)workspace);
    if (workspace_bytes < w.bytes) return fail(m, UU3D_ERR_WORKSPACE, "workspace smaller than uu3d_frame_features_bytes(frames)");
    uu3d_config c = m->cfg;
    if (exact_f32) c.precision = UU3D_PREC_F32;
    HIPCHK(m, hipSetDevice(m->device));
    Launcher Lh{m, (hipStream_t)stream_, w.slab, w.slab_floats, schedule == UU3D_SCHEDULE_THROUGHPUT, c.precision};
    m->prof_used = 0;
    const int dt = c.d_temporal;
    // stages 1-2 of the forward on a list of frames instead of B windows of N: no mask, no token blend, no PE
    spatial_stage(Lh, c, frames_dev, F, nullptr, nullptr, w.S, false, EpBias{features, m->s2t_b, dt});
    if (c.precision == UU3D_PREC_F16X3) {           // range guard (include/uu3d.h): non-finite features set the model's sticky word
        Lh.begin("range_check", "range_check", 0.0, 4.0 * (double)F * dt);
        hipLaunchKernelGGL(range_check_kernel, dim3(256), dim3(256), 0, Lh.stream, features, (long)F * dt, features, 0L, m->d_range);
        Lh.end();
    }
    return Lh.status;
}

// ---- operator ABI of stage 1 (include/uu3d_ops.h): the spatial kernels and the frame compaction on their own, through the helpers
// spatial_stage launches through -- tests/test_spatial_ops_gpu.py holds them to float64 ----
static_assert(UU3D_SPATIAL_AUTO == SPATIAL_AUTO && UU3D_SPATIAL_F32 == SPATIAL_F32 && UU3D_SPATIAL_H3_TILES == SPATIAL_H3_TILES && UU3D_SPATIAL_P16 == SPATIAL_P16,
              "uu3d_ops.h and uu3d_forward.inc name the spatial kernels alike");

// (a host query on a const handle: the status alone says what was wrong, the handle's last-error text is not written)
int uu3d_op_spatial_choice(const uu3d_model* m, int32_t F, int32_t schedule, int32_t* kernel, int32_t* planes) {
    if (!m || !kernel || !planes || F < 1) return UU3D_ERR_INVALID_ARGUMENT;
    const bool exact_f32 = (schedule & UU3D_SCHEDULE_EXACT_F32) != 0;
    schedule &= ~UU3D_SCHEDULE_EXACT_F32;
    if (schedule != UU3D_SCHEDULE_LATENCY && schedule != UU3D_SCHEDULE_THROUGHPUT) return UU3D_ERR_INVALID_ARGUMENT;
    if (m->generic) return UU3D_ERR_INVALID_ARGUMENT;      // a handle with generic dims has one spatial kernel
    uu3d_config c = m->cfg;
    if (exact_f32) c.precision = UU3D_PREC_F32;
    const SpatialChoice ch = spatial_choose(m, c, F);
    *kernel = ch.kernel; *planes = ch.planes ? 1 : 0;
    return UU3D_OK;
}

int uu3d_op_compact_frames(const uint8_t* mask_dev, int32_t total, int32_t* list_dev, void* stream) {
    if (!mask_dev || !list_dev || total < 1) return UU3D_ERR_INVALID_ARGUMENT;
    launch_compact_frames((hipStream_t)stream, mask_dev, total, list_dev);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_op_spatial_stack(uu3d_model* m, const float* frames_dev, int32_t F, const uint8_t* mask_dev, int32_t* frame_list_dev, int32_t kernel,
                          int32_t out_layout, void* out_dev, void* stream_) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    if (!frames_dev || !out_dev || F < 1) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_op_spatial_stack: null buffer or frames < 1");
    if (mask_dev != nullptr && frame_list_dev == nullptr) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_op_spatial_stack: a mask needs frame_list_dev (frames + 1 ints)");
    if (kernel < SPATIAL_AUTO || kernel > SPATIAL_P16) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_op_spatial_stack: unknown kernel");
    if (out_layout != UU3D_SPATIAL_OUT_F32 && out_layout != UU3D_SPATIAL_OUT_PLANES) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_op_spatial_stack: unknown output layout");
    if ((long)F * m->cfg.num_keypoints > (1L << 30)) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "too many frames");
    if (!m->committed) return fail(m, UU3D_ERR_NOT_READY, "uu3d_commit_weights has not been called");
    const bool want_planes = out_layout == UU3D_SPATIAL_OUT_PLANES;
    if (m->generic) {
        if (kernel != SPATIAL_AUTO) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_op_spatial_stack: the f32 / f16x3 spatial kernels are compiled for 17 joints, d_s 32, h_s 64, 8 heads; this handle has generic dims");
        if (mask_dev != nullptr) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_op_spatial_stack: spatial_generic_kernel takes no frame list");
        if (want_planes) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_op_spatial_stack: spatial_generic_kernel writes f32");
        if (!has_frames_form(m)) return no_frames_form(m, "uu3d_op_spatial_stack");
        return generic_op_spatial_stack(m, frames_dev, F, (float*)out_dev, stream_);
    }
    if (kernel == SPATIAL_AUTO) kernel = spatial_choose(m, m->cfg, F).kernel;
    if (kernel != SPATIAL_F32 && m->cfg.precision != UU3D_PREC_F16X3)
        return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_op_spatial_stack: a handle of precision f32 holds no f16 weight fragments for the f16x3 spatial kernels");
    if (kernel == SPATIAL_F32 && want_planes) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_op_spatial_stack: spatial_stack_mfma_kernel writes f32");
    HIPCHK(m, hipSetDevice(m->device));
    hipStream_t stream = (hipStream_t)stream_;
    if (mask_dev != nullptr) launch_compact_frames(stream, mask_dev, F, frame_list_dev);
    const size_t n = (size_t)F * m->cfg.num_keypoints * m->cfg.d_spatial;
    launch_spatial_stack(m, stream, kernel, frames_dev, F, mask_dev != nullptr ? frame_list_dev : nullptr, (float*)out_dev,      // (planes: hi over S, lo behind it, as spatial_stage places them)
                         want_planes ? (_Float16*)out_dev : nullptr, want_planes ? (_Float16*)out_dev + n : nullptr);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? UU3D_OK : fail(m, UU3D_ERR_HIP, std::string("uu3d_op_spatial_stack: launch failed: ") + hipGetErrorString(e));
}

// ---- the temporal chain, one launch on its own (uu3d_tchain16.h), through the helper Launcher::tchain launches through (launch_tchain,
// uu3d_launch.h), on the handle's own weight stream and parameter table -- tests/test_tchain_ops_gpu.py holds every stage set to float64 ----
size_t uu3d_op_tchain_scratch_bytes(int32_t M) { return M < 1 ? 0 : tchain16_scratch_bytes((M + 63) / 64); }

// (a host query on a const handle: the handle's last-error text is not written)  Returns the number of launches, -1 for a null handle or buffer
int uu3d_op_tchain_launches(const uu3d_model* m, int32_t* flags_out, int32_t capacity) {
    if (!m || capacity < 0 || (capacity > 0 && !flags_out)) return -1;
    if (!m->committed || m->generic || !tchain_possible(m->cfg)) return 0;
    for (size_t i = 0; i < m->tchain.size() && (int32_t)i < capacity; ++i) flags_out[i] = m->tchain[i].flags;
    return (int)m->tchain.size();
}

int uu3d_op_tchain(uu3d_model* m, int32_t launch, int32_t M, const void* attn_out_frag_dev, float* x_dev, float* xa_dev, void* q_dev, void* h_dev,
                   void* scratch_dev, void* stream_) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    if (M < 1 || launch < 0 || !scratch_dev) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_op_tchain: rows < 1, a negative launch or no scratch");
    if ((double)M * 1152 * 4.0 >= 4.0e9) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_op_tchain: too many rows");      // (the forward's limit for the chain)
    if (!m->committed) return fail(m, UU3D_ERR_NOT_READY, "uu3d_commit_weights has not been called");
    if (m->generic || !tchain_possible(m->cfg) || m->tchain.empty())
        return fail(m, UU3D_ERR_UNSUPPORTED, "uu3d_op_tchain: this handle has no temporal chain (precision f16x3, d_t 384, h_t 768, 8 heads, >= 1 temporal block)");
    if ((size_t)launch >= m->tchain.size()) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_op_tchain: no such launch");
    const uu3d_model::TcLaunch& t = m->tchain[launch];
    const int f = t.flags;
    const bool stores_x = (f & TC_MLP) != 0 && ((f & TC_QKV) == 0 || (f & TC_PE) != 0);      // (tchain16_kernel: the temporal stack's result)
    const float* pe = nullptr;
    if ((f & TC_PROJ) != 0 && !attn_out_frag_dev) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_op_tchain: this launch reads attn_out_frag_dev");
    if (((f & TC_PROJ) == 0 || stores_x) && !x_dev) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_op_tchain: this launch reads or writes x_dev");
    if ((f & TC_FC1_PLANES) != 0 && (!xa_dev || !h_dev)) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_op_tchain: this launch writes xa_dev and h_dev");
    if ((f & TC_QKV) != 0 && !q_dev) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_op_tchain: this launch writes q_dev");
    if ((f & TC_PE) != 0) {
        if (m->sblocks.empty() || m->sblocks[0].pe == nullptr || m->cfg.num_frames < 1) return fail(m, UU3D_ERR_UNSUPPORTED, "uu3d_op_tchain: no strided positional encoding");
        pe = m->sblocks[0].pe;
    }
    HIPCHK(m, hipSetDevice(m->device));
    const float qscale = 1.44269504088896341f / sqrtf((float)kDH);                          // = Launcher::attn_qscale()
    if (!launch_tchain((hipStream_t)stream_, f, M, m->harena + t.w_off, m->arena + t.p_off, qscale, (const _Float16*)attn_out_frag_dev, x_dev, xa_dev, pe,
                       (f & TC_PE) != 0 ? m->cfg.num_frames : 1, (_Float16*)q_dev, (_Float16*)h_dev, (unsigned char*)scratch_dev))
        return fail(m, UU3D_ERR_UNSUPPORTED, "temporal chain: unknown stage set");
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? UU3D_OK : fail(m, UU3D_ERR_HIP, std::string("uu3d_op_tchain: launch failed: ") + hipGetErrorString(e));
}
