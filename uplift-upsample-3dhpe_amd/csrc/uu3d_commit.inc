// uu3d_commit.inc -- uu3d_commit_weights: the host weights packed into the device operands of the forward (f32 arena, f16 hi / lo planes,
// fragment-ordered panels, the temporal chain's weight streams).  Included by uu3d_api.hip.
namespace {

// ---- host-side packing ------------------------------------------------------------------
struct Packer {
    std::vector<float> buf;
    std::vector<std::pair<size_t, size_t>> dense;  // (offset, floats) of every GEMM operand Bt[Np][Kp]
    size_t alloc(size_t n) {                       // 256-byte aligned segments
        size_t off = align_up(buf.size(), 64);
        buf.resize(off + n, 0.f);
        return off;
    }
    size_t alloc_dense(size_t n) { const size_t off = alloc(n); dense.emplace_back(off, n); return off; }
};

const float* W(const uu3d_model* m, const std::string& name) {
    auto it = m->index.find(name);
    return it == m->index.end() ? nullptr : m->weights[it->second].host.data();
}

// Keras Dense kernel (K, N) -> Bt[Np][Kp]: uu3d_pack.h (shared with the operator ABI)
void pack_dense_t(std::vector<float>& buf, size_t off, const float* w, int K, int N, int Kp, int n0) { uu3d::pack_dense_t(buf.data(), off, w, K, N, Kp, n0); }

}  // namespace

int uu3d_commit_weights(uu3d_model* m, void* stream_) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    for (auto& r : m->weights)
        if (!r.set) return fail(m, UU3D_ERR_NOT_READY, "weight never set: " + r.name);
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(m, hipSetDevice(m->device));
    if (m->generic) {
        // generic dims: the forward reads the master buffer and the operand packs of the training-mode chain (uu3d_train_init; called again it
        // re-uploads the weights and repacks)
        if (m->gparams == nullptr) {
            long long n = 0;
            for (auto& r : m->weights) n += r.numel;
            HIPCHK(m, hipMalloc((void**)&m->gparams, (size_t)n * sizeof(float)));
        }
        m->in_commit = true;
        const int r = uu3d_train_init(m, m->gparams, stream_);
        m->in_commit = false;
        if (r != UU3D_OK) return r;
        HIPCHK(m, hipStreamSynchronize(stream));
        m->committed = true;
        return UU3D_OK;
    }
    const uu3d_config& c = m->cfg;
    const int J = c.num_keypoints, N = c.num_frames, ds = c.d_spatial, dt = c.d_temporal, ht = c.h_temporal;
    const int Kdt = round_up(dt, 32), Kht = round_up(ht, 32), Ks2t = round_up(J * ds, 32);
    Packer P;

    // ---- spatial ----
    const size_t o_ew = P.alloc(2 * ds), o_eb = P.alloc(ds), o_spe = P.alloc((size_t)J * ds);
    std::copy_n(W(m, "keypoint_embedding/kernel"), 2 * ds, P.buf.begin() + o_ew);
    std::copy_n(W(m, "keypoint_embedding/bias"), ds, P.buf.begin() + o_eb);
    std::copy_n(W(m, "spatial_pe/positional_encoding_weights"), J * ds, P.buf.begin() + o_spe);
    const size_t o_sblk = P.alloc((size_t)c.spatial_depth * SLY2::size);
    for (int i = 0; i < c.spatial_depth; ++i) {
        const std::string p = "spatial_block_" + std::to_string(i + 1);
        float* d = P.buf.data() + o_sblk + (size_t)i * SLY2::size;
        auto vec = [&](int off, const std::string& nm, int n) {
            const float* s = W(m, p + nm);
            if (s) std::copy_n(s, n, d + off);
        };
        // fragment order of the 32x32x2 MFMA B operand: [n-tile][kk][lane][s] = W[8kk + 4(lane>>5) + s][32nt + (lane&31)]
        auto frag = [&](int off, const std::string& nm, int K, int Nn) {
            const float* s = W(m, p + nm);
            for (int nt = 0; nt < Nn / 32; ++nt)
                for (int kk = 0; kk < K / 8; ++kk)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 4; ++e)
                            d[off + ((nt * (K / 8) + kk) * 64 + lane) * 4 + e] =
                                s[(size_t)(8 * kk + 4 * (lane >> 5) + e) * Nn + 32 * nt + (lane & 31)];
        };
        vec(SLY2::ln1_g, "/norm1/gamma", ds); vec(SLY2::ln1_b, "/norm1/beta", ds);
        vec(SLY2::ln2_g, "/norm2/gamma", ds); vec(SLY2::ln2_b, "/norm2/beta", ds);
        vec(SLY2::bq, "/attn/wq/bias", ds); vec(SLY2::bk, "/attn/wk/bias", ds); vec(SLY2::bv, "/attn/wv/bias", ds);
        vec(SLY2::bp, "/attn/projection/bias", ds); vec(SLY2::b1, "/mlp/fc1/bias", kHS); vec(SLY2::b2, "/mlp/fc2/bias", ds);
        frag(SLY2::fq, "/attn/wq/kernel", ds, ds); frag(SLY2::fk, "/attn/wk/kernel", ds, ds);
        frag(SLY2::fv, "/attn/wv/kernel", ds, ds); frag(SLY2::fp, "/attn/projection/kernel", ds, ds);
        frag(SLY2::f1, "/mlp/fc1/kernel", ds, kHS); frag(SLY2::f2, "/mlp/fc2/kernel", kHS, ds);
    }
    const size_t o_sng = P.alloc(ds), o_snb = P.alloc(ds);
    std::copy_n(W(m, "spatial_norm/gamma"), ds, P.buf.begin() + o_sng);
    std::copy_n(W(m, "spatial_norm/beta"), ds, P.buf.begin() + o_snb);

    // ---- spatial_to_temporal_fc, token, temporal PE ----
    const int Npdt = round_up(dt, 128);
    const size_t o_s2t = P.alloc_dense((size_t)Npdt * Ks2t), o_s2tb = P.alloc(Npdt);
    pack_dense_t(P.buf, o_s2t, W(m, "spatial_to_temporal_fc/kernel"), J * ds, dt, Ks2t, 0);
    std::copy_n(W(m, "spatial_to_temporal_fc/bias"), dt, P.buf.begin() + o_s2tb);
    const size_t o_tok = P.alloc(dt);
    if (c.has_strided_input)
        std::copy_n(W(m, "strided_input_token_layer/learnable_masked_token"), dt, P.buf.begin() + o_tok);
    const size_t o_pet = P.alloc((size_t)N * dt);
    std::copy_n(W(m, "temporal_pe/positional_encoding_weights"), (size_t)N * dt, P.buf.begin() + o_pet);

    // ---- transformer blocks ----
    struct BlockOff { size_t ln1_g, ln1_b, wqkv, bqkv, wp, bp, ln2_g, ln2_b, w1, b1, w2, b2, pe; };
    auto pack_block = [&](const std::string& p, bool strided, int peL, const std::string& pe_name) {
        BlockOff o{};
        o.ln1_g = P.alloc(dt); o.ln1_b = P.alloc(dt);
        std::copy_n(W(m, p + "/norm1/gamma"), dt, P.buf.begin() + o.ln1_g);
        std::copy_n(W(m, p + "/norm1/beta"), dt, P.buf.begin() + o.ln1_b);
        const int Npq = round_up(3 * dt, 128);
        o.wqkv = P.alloc_dense((size_t)Npq * Kdt); o.bqkv = P.alloc(Npq);
        int part = 0;
        for (const char* nm : {"wq", "wk", "wv"}) {
            pack_dense_t(P.buf, o.wqkv, W(m, p + "/attn/" + nm + "/kernel"), dt, dt, Kdt, part * dt);
            const float* b = W(m, p + "/attn/" + nm + "/bias");
            if (b) std::copy_n(b, dt, P.buf.begin() + o.bqkv + part * dt);
            ++part;
        }
        o.wp = P.alloc_dense((size_t)Npdt * Kdt); o.bp = P.alloc(Npdt);
        pack_dense_t(P.buf, o.wp, W(m, p + "/attn/projection/kernel"), dt, dt, Kdt, 0);
        std::copy_n(W(m, p + "/attn/projection/bias"), dt, P.buf.begin() + o.bp);
        o.ln2_g = P.alloc(dt); o.ln2_b = P.alloc(dt);
        std::copy_n(W(m, p + "/norm2/gamma"), dt, P.buf.begin() + o.ln2_g);
        std::copy_n(W(m, p + "/norm2/beta"), dt, P.buf.begin() + o.ln2_b);
        const int Nph = round_up(ht, 128);
        o.w1 = P.alloc_dense((size_t)Nph * Kdt); o.b1 = P.alloc(Nph);
        pack_dense_t(P.buf, o.w1, W(m, p + "/mlp/fc1/kernel"), dt, ht, Kdt, 0);   // Conv1D k=1 (1,dt,ht) has the same flat layout
        std::copy_n(W(m, p + "/mlp/fc1/bias"), ht, P.buf.begin() + o.b1);
        if (strided) {
            const int Kc = round_up(3 * ht, 32);
            o.w2 = P.alloc_dense((size_t)Npdt * Kc); o.b2 = P.alloc(Npdt);
            // Conv1D kernel (3, ht, dt): flat (j*ht + c, n) is exactly a Dense kernel of K = 3*ht
            pack_dense_t(P.buf, o.w2, W(m, p + "/mlp/strided_conv/kernel"), 3 * ht, dt, Kc, 0);
            std::copy_n(W(m, p + "/mlp/strided_conv/bias"), dt, P.buf.begin() + o.b2);
            o.pe = P.alloc((size_t)peL * dt);
            std::copy_n(W(m, pe_name), (size_t)peL * dt, P.buf.begin() + o.pe);
        } else {
            o.w2 = P.alloc_dense((size_t)Npdt * Kht); o.b2 = P.alloc(Npdt);
            pack_dense_t(P.buf, o.w2, W(m, p + "/mlp/fc2/kernel"), ht, dt, Kht, 0);
            std::copy_n(W(m, p + "/mlp/fc2/bias"), dt, P.buf.begin() + o.b2);
        }
        return o;
    };
    std::vector<BlockOff> toff, soff;
    for (int i = 0; i < c.temporal_depth; ++i)
        toff.push_back(pack_block("temporal_block_" + std::to_string(i + 1), false, 0, ""));
    for (int i = 0; i < c.num_strided; ++i)
        soff.push_back(pack_block("strided_temporal_block_" + std::to_string(i + 1), true, m->L[i],
                                  "strided_temporal_pe_" + std::to_string(i + 1) + "/positional_encoding_weights"));

    // ---- heads ----
    const int Nph = round_up(3 * J, 128);
    size_t o_h1 = 0, o_h1b = 0;
    const bool has_h1 = c.full_output && c.temporal_depth > 0;
    // OUTPUT_BN at inference (u_u_t.py:275-285, Keras BatchNormalization with training=False): y = gamma (x - mean) / sqrt(var + eps) + beta
    // is a per-channel affine in front of the Dense head, so it is folded into the head's operands here:
    //   W'[k][n] = s[k] W[k][n],  b'[n] = b[n] + sum_k (beta[k] - mean[k] s[k]) W[k][n],  s = gamma / sqrt(var + 1e-5)
    auto pack_head = [&](size_t o_w, size_t o_b, const std::string& fc, const std::string& bn) {
        const float* Wk = W(m, fc + "/kernel"); const float* bk = W(m, fc + "/bias");
        if (!c.output_bn) {
            pack_dense_t(P.buf, o_w, Wk, dt, 3 * J, Kdt, 0);
            std::copy_n(bk, 3 * J, P.buf.begin() + o_b);
            return;
        }
        const float *g = W(m, bn + "/gamma"), *be = W(m, bn + "/beta"), *mu = W(m, bn + "/moving_mean"), *var = W(m, bn + "/moving_variance");
        std::vector<float> Wf((size_t)dt * 3 * J);
        std::vector<double> bf(3 * J);
        for (int n = 0; n < 3 * J; ++n) bf[n] = bk[n];
        for (int k = 0; k < dt; ++k) {
            const float s = g[k] / std::sqrt(var[k] + 1e-5f);
            const double sh = (double)be[k] - (double)mu[k] * s;
            for (int n = 0; n < 3 * J; ++n) { Wf[(size_t)k * 3 * J + n] = s * Wk[(size_t)k * 3 * J + n]; bf[n] += sh * Wk[(size_t)k * 3 * J + n]; }
        }
        pack_dense_t(P.buf, o_w, Wf.data(), dt, 3 * J, Kdt, 0);
        for (int n = 0; n < 3 * J; ++n) P.buf[o_b + n] = (float)bf[n];
    };
    if (has_h1) {
        o_h1 = P.alloc_dense((size_t)Nph * Kdt); o_h1b = P.alloc(Nph);
        pack_head(o_h1, o_h1b, "temporal_fc", "temporal_norm");
    }
    const size_t o_h2 = P.alloc_dense((size_t)Nph * Kdt), o_h2b = P.alloc(Nph);
    pack_head(o_h2, o_h2b, "strided_temporal_fc", "strided_temporal_norm");

    // ---- temporal chain (uu3d_tchain16.h): per launch one parameter table (floats) and one weight stream (f16 planes, built below) ----
    // A LayerNorm's affine part is folded into the Dense layer behind it: W' = diag(gamma) W, b' = b + beta W (f64 sums).
    const float tc_qscale = 1.44269504088896341f / sqrtf((float)(dt / std::max(1, c.num_heads)));      // = Launcher::attn_qscale(): log2(e) / sqrt(d_h)
    struct TcStage { std::vector<float> Wk; int K, N, kofs; bool natural; };        // Keras layout [K][N]
    struct TcBuild { int flags; size_t p_off; std::vector<TcStage> stages; };
    std::vector<TcBuild> tcb;
    if (tchain_possible(c)) {
        auto block_name = [&](bool strided, int i) { return std::string(strided ? "strided_temporal_block_" : "temporal_block_") + std::to_string(i + 1); };
        auto folded = [&](const std::vector<float>& Wk, const std::vector<float>& b, const float* g, const float* be, int K, int Nn, std::vector<float>& bout) {
            TcStage st{std::vector<float>((size_t)K * Nn), K, Nn, 0, false};
            bout.assign(Nn, 0.f);
            for (int n = 0; n < Nn; ++n) { double acc = b[n]; for (int k = 0; k < K; ++k) acc += (double)be[k] * Wk[(size_t)k * Nn + n]; bout[n] = (float)acc; }
            for (int k = 0; k < K; ++k) for (int n = 0; n < Nn; ++n) st.Wk[(size_t)k * Nn + n] = g[k] * Wk[(size_t)k * Nn + n];
            return st;
        };
        auto qkv_of = [&](const std::string& p, std::vector<float>& Wk, std::vector<float>& b) {       // wq | wk | wv as one (dt, 3 dt) kernel
            Wk.assign((size_t)dt * 3 * dt, 0.f); b.assign(3 * dt, 0.f);
            int part = 0;
            for (const char* nm : {"wq", "wk", "wv"}) {
                const float* w = W(m, p + "/attn/" + nm + "/kernel"); const float* bb = W(m, p + "/attn/" + nm + "/bias");
                for (int k = 0; k < dt; ++k) for (int n = 0; n < dt; ++n) Wk[(size_t)k * 3 * dt + part * dt + n] = w[(size_t)k * dt + n];
                if (bb) std::copy_n(bb, dt, b.begin() + part * dt);
                ++part;
            }
        };
        auto add_qkv = [&](TcBuild& tb, const std::string& p) {
            std::vector<float> Wk, b, bf; qkv_of(p, Wk, b);
            tb.stages.push_back(folded(Wk, b, W(m, p + "/norm1/gamma"), W(m, p + "/norm1/beta"), dt, 3 * dt, bf));
            for (int n = 0; n < dt; ++n) bf[n] *= tc_qscale;          // (q's scale is folded into wq and bq)
            std::copy_n(bf.begin(), 3 * dt, P.buf.begin() + tb.p_off + TCP_BQKV);
        };
        auto add_proj = [&](TcBuild& tb, const std::string& p) {
            const float* w = W(m, p + "/attn/projection/kernel");
            tb.stages.push_back(TcStage{std::vector<float>(w, w + (size_t)dt * dt), dt, dt, 0, true});
            std::copy_n(W(m, p + "/attn/projection/bias"), dt, P.buf.begin() + tb.p_off + TCP_BP);
        };
        auto add_fc1 = [&](TcBuild& tb, const std::string& p) {
            const float* w = W(m, p + "/mlp/fc1/kernel"); const float* b = W(m, p + "/mlp/fc1/bias");
            std::vector<float> bf;
            tb.stages.push_back(folded(std::vector<float>(w, w + (size_t)dt * ht), std::vector<float>(b, b + ht), W(m, p + "/norm2/gamma"), W(m, p + "/norm2/beta"), dt, ht, bf));
            std::copy_n(bf.begin(), ht, P.buf.begin() + tb.p_off + TCP_B1);
        };
        auto add_fc2 = [&](TcBuild& tb, const std::string& p) {
            const float* w = W(m, p + "/mlp/fc2/kernel");
            for (int half = 0; half < 2; ++half) tb.stages.push_back(TcStage{std::vector<float>(w, w + (size_t)ht * dt), ht, dt, half * dt, false});
            std::copy_n(W(m, p + "/mlp/fc2/bias"), dt, P.buf.begin() + tb.p_off + TCP_B2);
        };
        { TcBuild tb{TC_QKV, P.alloc(TCP_FLOATS), {}}; add_qkv(tb, block_name(false, 0)); tcb.push_back(std::move(tb)); }
        for (int i = 0; i < c.temporal_depth; ++i) {
            const bool last = i + 1 == c.temporal_depth;
            TcBuild tb{TC_PROJ | TC_MLP | (last ? (c.num_strided > 0 ? TC_QKV | TC_PE : 0) : TC_QKV), P.alloc(TCP_FLOATS), {}};
            add_proj(tb, block_name(false, i)); add_fc1(tb, block_name(false, i)); add_fc2(tb, block_name(false, i));
            if (!last) add_qkv(tb, block_name(false, i + 1)); else if (c.num_strided > 0) add_qkv(tb, block_name(true, 0));
            tcb.push_back(std::move(tb));
        }
        if (c.num_strided > 0) {
            TcBuild tb{TC_PROJ | TC_FC1_PLANES, P.alloc(TCP_FLOATS), {}};
            add_proj(tb, block_name(true, 0)); add_fc1(tb, block_name(true, 0));
            tcb.push_back(std::move(tb));
        }
    }

    // ---- upload ----
    if (m->arena_floats < P.buf.size()) {
        if (m->arena) HIPCHK(m, hipFree(m->arena));
        m->arena = nullptr;
        HIPCHK(m, hipMalloc((void**)&m->arena, P.buf.size() * sizeof(float)));
        m->arena_floats = P.buf.size();
    }
    HIPCHK(m, hipMemcpyAsync(m->arena, P.buf.data(), P.buf.size() * sizeof(float), hipMemcpyHostToDevice, stream));
    HIPCHK(m, hipStreamSynchronize(stream));
    if (c.precision == UU3D_PREC_F16X3) {
        // split every GEMM operand into f16 hi / (lo * 2048) planes (uu3d_gemm_h3.h)
        std::vector<_Float16> hb(64, (_Float16)0.f);      // [0, 64): zeros, the source of out-of-range conv taps (GLoadConv3)
        m->hplanes.clear();
        for (auto& d : P.dense) {
            const size_t hi = align_up(hb.size(), 64); hb.resize(hi + d.second);
            const size_t lo = align_up(hb.size(), 64); hb.resize(lo + d.second);
            if (!split_operand_planes(P.buf.data() + d.first, d.second, hb.data() + hi, hb.data() + lo))      // (uu3d_pack.h; include/uu3d.h, RANGE CONTRACT: the hi plane of such a weight is Inf)
                return fail(m, UU3D_ERR_RANGE, "a Dense / Conv1D kernel holds a value of magnitude >= 65504 (or a non-finite one): not representable by the f16x3 operand planes; build the model with precision f32");
            m->hplanes[d.first] = {hi, lo};
        }
        {   // spatial stack: A-operand fragments of W^T (uu3d_spatial_h3.h), [n-tile][kk][plane][lane][8]
            using FL = SpatialFragLayoutH3;
            m->sp_frag_off = align_up(hb.size(), 64);
            hb.resize(m->sp_frag_off + (size_t)c.spatial_depth * FL::size);
            for (int i = 0; i < c.spatial_depth; ++i) {
                const std::string p = "spatial_block_" + std::to_string(i + 1);
                _Float16* d = hb.data() + m->sp_frag_off + (size_t)i * FL::size;
                auto frag = [&](int off, const std::string& nm, int K, int Nn) {
                    const float* s = W(m, p + nm);
                    for (int nt = 0; nt < Nn / 32; ++nt)
                        for (int kk = 0; kk < K / 16; ++kk)
                            for (int lane = 0; lane < 64; ++lane)
                                for (int e = 0; e < 8; ++e) {
                                    const float x = s[(size_t)(16 * kk + 8 * (lane >> 5) + e) * Nn + 32 * nt + (lane & 31)];
                                    const _Float16 h = h3_hi(x);
                                    const size_t at = (size_t)off + (((size_t)(nt * (K / 16) + kk) * 2) * 64 + lane) * 8 + e;
                                    d[at] = h;
                                    d[at + 64 * 8] = (_Float16)((x - (float)h) * H3_SCALE);
                                }
                };
                frag(FL::fq, "/attn/wq/kernel", ds, ds); frag(FL::fk, "/attn/wk/kernel", ds, ds);
                frag(FL::fv, "/attn/wv/kernel", ds, ds); frag(FL::fp, "/attn/projection/kernel", ds, ds);
                frag(FL::f1, "/mlp/fc1/kernel", ds, kHS); frag(FL::f2, "/mlp/fc2/kernel", kHS, ds);
            }
        }
        {   // the same matrices for spatial_stack_p16_kernel (uu3d_spatial_p16.h): [n-tile 16][k-step 32][plane][lane][8], k in p16_kch order
            using FL = SpatialFragLayoutP16;
            m->sp_frag16_off = align_up(hb.size(), 64);
            hb.resize(m->sp_frag16_off + (size_t)c.spatial_depth * FL::size);
            for (int i = 0; i < c.spatial_depth; ++i) {
                const std::string p = "spatial_block_" + std::to_string(i + 1);
                _Float16* d = hb.data() + m->sp_frag16_off + (size_t)i * FL::size;
                auto frag = [&](int off, const std::string& nm, int K, int Nn) {
                    const float* s = W(m, p + nm);
                    for (int nt = 0; nt < Nn / 16; ++nt)
                        for (int ks = 0; ks < K / 32; ++ks)
                            for (int lane = 0; lane < 64; ++lane)
                                for (int j = 0; j < 8; ++j) {
                                    const float x = s[(size_t)p16_kch(ks, lane >> 4, j) * Nn + 16 * nt + (lane & 15)];
                                    const _Float16 h = h3_hi(x);
                                    const size_t at = (size_t)off + (((size_t)(nt * (K / 32) + ks) * 2) * 64 + lane) * 8 + j;
                                    d[at] = h;
                                    d[at + 64 * 8] = (_Float16)((x - (float)h) * H3_SCALE);
                                }
                };
                frag(FL::fq, "/attn/wq/kernel", ds, ds); frag(FL::fk, "/attn/wk/kernel", ds, ds);
                frag(FL::fv, "/attn/wv/kernel", ds, ds); frag(FL::fp, "/attn/projection/kernel", ds, ds);
                frag(FL::f1, "/mlp/fc1/kernel", ds, kHS); frag(FL::f2, "/mlp/fc2/kernel", kHS, ds);
            }
        }
        // row-panel GEMM operands (uu3d_gemm_panel.h): wqkv and w1 of every temporal / strided block, fragment ordered
        m->panel_off.clear();
        if (dt % 192 == 0 && ht % 32 == 0) {
            auto add_panel = [&](size_t bt_off, int Nn, int K = 0, int Kp = 0) {
                if (K == 0) { K = dt; Kp = Kdt; }
                const auto it = m->hplanes.find(bt_off);
                if (it == m->hplanes.end() || K % 384 != 0) return;
                const size_t at = align_up(hb.size(), 64);
                hb.resize(at + panel_b_halfs(Nn, K));
                panel_pack_operand(hb.data() + it->second.first, hb.data() + it->second.second, Nn, K, Kp, hb.data() + at);
                m->panel_off[bt_off] = at;
            };
            for (auto& o : toff) { add_panel(o.wqkv, 3 * dt); add_panel(o.w1, ht); add_panel(o.wp, dt); }
            // fused MLP (uu3d_mlp_fused.h): fc2 fragments in the k order fc1's accumulator registers have
            m->mlpf_off.clear();
            if (dt == 32 * MLPF_OC && ht == 256 * MLPF_SLICES)
                for (auto& o : toff) {
                    const auto it = m->hplanes.find(o.w2);
                    if (it == m->hplanes.end()) continue;
                    const size_t at = align_up(hb.size(), 64);
                    hb.resize(at + mlpf_w2_halfs());
                    mlpf_pack_w2(hb.data() + it->second.first, hb.data() + it->second.second, Kht, hb.data() + at);
                    m->mlpf_off[o.w2] = at;
                }
            for (auto& o : soff) { add_panel(o.wqkv, 3 * dt); add_panel(o.w1, ht); add_panel(o.wp, dt); }
        }
        // temporal chain: the launches' weight streams (tchain16_pack_stage: one 48 KiB chunk per 32 output channels and stage)
        m->tchain.clear();
        for (auto& tb : tcb) {
            const size_t at = align_up(hb.size(), 128);
            hb.resize(at + (size_t)tchain_chunks(tb.flags) * TC_CHUNK_HALFS);
            size_t o = at;
            for (auto& st : tb.stages) {
                std::vector<_Float16> Bh((size_t)st.N * st.K), Bl((size_t)st.N * st.K);
                const bool qkv_stage = st.N == 3 * dt;                 // (q's scale lives in wq and bq)
                for (int n = 0; n < st.N; ++n)
                    for (int k = 0; k < st.K; ++k) {
                        const float x = st.Wk[(size_t)k * st.N + n] * (qkv_stage && n < dt ? tc_qscale : 1.0f);
                        if (!(std::fabs(x) < 65504.0f)) return fail(m, UU3D_ERR_RANGE, "a LayerNorm-folded kernel of the temporal chain leaves the f16 range; build the model with precision f32");
                        const _Float16 h = h3_hi(x);
                        Bh[(size_t)n * st.K + k] = h; Bl[(size_t)n * st.K + k] = (_Float16)((x - (float)h) * H3_SCALE);
                    }
                tchain16_pack_stage(Bh.data(), Bl.data(), st.N, st.K, st.kofs, st.natural, hb.data() + o);
                o += (size_t)(st.N / 32) * TC_CHUNK_HALFS;
            }
            if (tb.flags & TC_MLP) {                                // W1 (24 chunks) | W2 half 0 | W2 half 1  ->  W1[0..11] | W2 half 0 | W1[12..23] | W2 half 1
                _Float16* mlp = hb.data() + at + (size_t)((tb.flags & TC_PROJ) ? 12 : 0) * TC_CHUNK_HALFS;
                const std::vector<_Float16> tmp(mlp, mlp + (size_t)48 * TC_CHUNK_HALFS);
                tchain16_reorder_mlp(tmp.data(), mlp);
            }
            m->tchain.push_back({tb.flags, at, tb.p_off});
        }
        if (m->harena_halfs < hb.size()) {
            if (m->harena) HIPCHK(m, hipFree(m->harena));
            m->harena = nullptr;
            HIPCHK(m, hipMalloc((void**)&m->harena, hb.size() * sizeof(_Float16)));
            m->harena_halfs = hb.size();
        }
        HIPCHK(m, hipMemcpyAsync(m->harena, hb.data(), hb.size() * sizeof(_Float16), hipMemcpyHostToDevice, stream));
        HIPCHK(m, hipStreamSynchronize(stream));
    }

    const float* A = m->arena;
    m->sp.embed_w = A + o_ew; m->sp.embed_b = A + o_eb; m->sp.pe = A + o_spe; m->sp.blocks = A + o_sblk;
    m->sp.norm_g = A + o_sng; m->sp.norm_b = A + o_snb; m->sp.depth = c.spatial_depth; m->sp.total_frames = 0;
    m->s2t_wt = A + o_s2t; m->s2t_b = A + o_s2tb; m->token = A + o_tok; m->pe_t = A + o_pet;
    auto view = [&](const BlockOff& o, bool strided) {
        BlockDev b{};
        b.ln1_g = A + o.ln1_g; b.ln1_b = A + o.ln1_b; b.wqkv_t = A + o.wqkv; b.bqkv = A + o.bqkv;
        b.wp_t = A + o.wp; b.bp = A + o.bp; b.ln2_g = A + o.ln2_g; b.ln2_b = A + o.ln2_b;
        b.w1_t = A + o.w1; b.b1 = A + o.b1; b.w2_t = A + o.w2; b.b2 = A + o.b2;
        b.pe = strided ? A + o.pe : nullptr;
        { const auto it = m->panel_off.find(o.wqkv); b.wqkv_pf = (it != m->panel_off.end()) ? it->second : 0; }
        { const auto it = m->panel_off.find(o.w1); b.w1_pf = (it != m->panel_off.end()) ? it->second : 0; }
        { const auto it = m->mlpf_off.find(o.w2); b.w2_mf = (!strided && it != m->mlpf_off.end()) ? it->second : 0; }
        { const auto it = m->panel_off.find(o.wp); b.wp_pf = (it != m->panel_off.end()) ? it->second : 0; }
        return b;
    };
    m->tblocks.clear(); m->sblocks.clear();
    for (auto& o : toff) m->tblocks.push_back(view(o, false));
    for (auto& o : soff) m->sblocks.push_back(view(o, true));
    m->h1_wt = has_h1 ? A + o_h1 : nullptr; m->h1_b = has_h1 ? A + o_h1b : nullptr;
    m->h2_wt = A + o_h2; m->h2_b = A + o_h2b;
    m->committed = true;
    return UU3D_OK;
}
