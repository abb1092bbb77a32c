// uu3d_api.hip -- C ABI (include/uu3d.h) over the gfx950 kernels: the model object, the weight inventory, create / destroy, weight
// get / set and the small entry points.  One translation unit with
//   uu3d_commit.inc      uu3d_commit_weights: host weights -> packed device operands
//   uu3d_forward.inc     workspace, Launcher, the forward launch schedule (uu3d_forward*, uu3d_frame_features)
//   uu3d_train_state.inc, uu3d_train_forward.inc, uu3d_train_backward.inc, uu3d_train_entry.inc
//                        the training step: state / init / repack / carve, the forward, the backward with its side streams, the entry points and the tape
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/uu3d.h"
#include "../../include/uu3d_ops.h"      // the operators that need the model: uu3d_op_spatial_* (uu3d_forward.inc)
#include "uu3d_switches.h"
#include "uu3d_gemm.h"
#include "uu3d_gemm_h3.h"
#include "uu3d_pack.h"
#include "uu3d_gemm_panel.h"
#include "uu3d_gemm_panel8.h"
#include "uu3d_gemm_wt.h"
#include "uu3d_mlp_fused.h"
#include "uu3d_tchain16.h"
#include "uu3d_attn.h"
#include "uu3d_attn_h3.h"
#include "uu3d_spatial.h"
#include "uu3d_spatial_h3.h"
#include "uu3d_spatial_p16.h"
#include "uu3d_spatial_generic.h"
#include "uu3d_misc.h"
#include "uu3d_metrics.h"
#include "uu3d_tracks.h"
#include "uu3d_repair.h"
#include "uu3d_root.h"
#include "uu3d_keypoints.h"
#include "uu3d_associate.h"
#include "uu3d_stream.h"
#include "uu3d_stream_rate.h"
#include "uu3d_stream_repair.h"
#include "uu3d_stream_root.h"
#include "uu3d_stream_drain.h"
#include "uu3d_smooth.h"
#include "uu3d_bones.h"
#include "uu3d_rotations.h"
#include "uu3d_undistort.h"
#include "uu3d_world.h"
#include "uu3d_views.h"
#include "uu3d_view_match.h"
#include "uu3d_view_align.h"
#include "uu3d_triangulate.h"
#include "uu3d_view_calibrate.h"
#include "uu3d_lift_match.h"
#include "uu3d_stream_views.h"
#include "uu3d_train.h"
#include "uu3d_bwd.h"
#include "uu3d_launch.h"
#include "uu3d_train_kernels.h"

using namespace uu3d;

namespace {

constexpr int kJ = 17, kDS = 32, kHS = 64, kHeads = 8, kDH = 48;
using SLY2 = SpatialBlockLayoutV2<kDS, kHS>;
constexpr int kFR = 3;   // frames per wave in the MFMA spatial kernel (3 * 17 = 51 rows)
#ifndef UU3D_SPATIAL_MT
#define UU3D_SPATIAL_MT 1
#endif
constexpr int kP16FR = 7, kP16PW = 1;   // spatial_stack_p16_kernel: 7 frames = 119 tokens on 8 waves of one 16-token panel (uu3d_spatial_p16.h)
constexpr int kSpatialMT = UU3D_SPATIAL_MT;   // token tiles per wave of the f16x3 spatial kernel: 1 = two waves per 3 frames (see uu3d_spatial_h3.h)

std::string g_create_error;

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct WeightRec {
    std::string name;
    std::vector<int64_t> dims;
    int64_t numel = 0;
    std::vector<float> host;
    bool set = false;
};

// Device views of one packed transformer block (temporal or strided).
struct BlockDev {
    const float *ln1_g, *ln1_b, *wqkv_t, *bqkv, *wp_t, *bp, *ln2_g, *ln2_b, *w1_t, *b1, *w2_t, *b2;
    const float* pe;   // strided blocks: (L_i, d_t)
    // fragment-ordered f16 planes of wqkv / w1 for the row-panel GEMM (uu3d_gemm_panel.h); offsets in harena, 0 = none
    size_t wqkv_pf = 0, w1_pf = 0;
    size_t w2_mf = 0;                  // fc2 fragments of the fused MLP kernel (uu3d_mlp_fused.h, temporal blocks), offset in harena, 0 = none
    size_t wp_pf = 0;                  // fragment-ordered projection operand (row-panel GEMM), 0 = none
};

struct ProfRec {
    std::string name, kernel;
    double flops, bytes;
    hipEvent_t e0, e1;
};

}  // namespace

struct uu3d_train_state;
struct uu3d_model {
    uu3d_config cfg;
    uu3d_train_state* ts = nullptr;   // training packs (uu3d_train_init)
    int device = 0;
    std::vector<WeightRec> weights;
    std::map<std::string, int> index;
    std::vector<int> L;            // strided lengths L_0 .. L_ns
    Switches sw;                   // the environment switches of this handle (uu3d_switches.h), read by uu3d_create
    bool committed = false;
    // Dims other than the compiled ones (J = 17, d_s = 32, h_s = 64, 8 heads, d_t = 384): the forward runs on the GENERIC kernels of the
    // training-mode chain (uu3d_train_forward.inc: tiled GEMMs with LayerNorm / GELU loaders, attn_generic_fwd_kernel, one launch per layer)
    // from a master buffer the model owns -- correct and an order of magnitude slower than the specialised path; no backward pass.
    bool generic = false;
    float* gparams = nullptr;      // generic: master parameter buffer (uu3d_train_init layout)
    float* arena = nullptr;        // packed device weights
    size_t arena_floats = 0;
    bool throughput = false;       // uu3d_set_schedule: launches shaped for CU-microseconds (several forwards share the chip) instead of latency
    // Temporal chain (uu3d_tchain16.h; throughput schedule): one launch per temporal block for its row-local stages.  Launch 0 = LayerNorm 1 + QKV of
    // block 1; launch i (1 .. T) = projection + MLP of block i (+ LayerNorm 1 + QKV of the block behind it: temporal block i + 1, or the first strided
    // block with its positional encoding); launch T + 1 = projection + LayerNorm 2 + fc1 of the first strided block.  Empty = not available.
    struct TcLaunch { int flags; size_t w_off /* halfs, harena */; size_t p_off /* floats, arena */; };
    std::vector<TcLaunch> tchain;
    int num_cus = 256;
    std::recursive_mutex train_mu; // the training-mode chain keeps per-call options in the handle's training state (uu3d_train_state.inc): one call at a time
    bool in_commit = false;        // uu3d_commit_weights is calling uu3d_train_init (generic dims): the training step's skip flag is not its to clear
    int* d_range = nullptr;        // sticky device word of the range guard (include/uu3d.h: uu3d_range_status)
    _Float16* harena = nullptr;    // f16 hi/lo planes of every GEMM operand (f16x3 mode)
    size_t harena_halfs = 0;
    std::map<size_t, std::pair<size_t, size_t>> hplanes;   // Bt float offset -> (hi offset, lo offset) in harena
    std::map<size_t, size_t> panel_off, mlpf_off;          // mlpf_off: Bt float offset of fc2 -> mlpf_pack_w2 fragments in harena                    // Bt float offset -> fragment-ordered planes in harena (uu3d_gemm_panel.h)
    // packed views
    SpatialParams sp{};            // (blocks: SpatialBlockLayoutV2, the layout of every spatial kernel of the forward)
    size_t sp_frag_off = 0;        // offset (halfs) of the spatial f16 fragment planes in harena
    size_t sp_frag16_off = 0;      // the same in the 16-token-panel order of spatial_stack_p16_kernel
    const float *s2t_wt = nullptr, *s2t_b = nullptr, *token = nullptr, *pe_t = nullptr;
    std::vector<BlockDev> tblocks, sblocks;
    const float *h1_wt = nullptr, *h1_b = nullptr, *h2_wt = nullptr, *h2_b = nullptr;
    // profiling
    bool profiling = false;
    std::vector<ProfRec> prof;
    size_t prof_used = 0;
    std::string err;
};

namespace {

// (a property of the configuration, not of the commit state: uu3d_workspace_bytes may be asked before the weights are committed)
inline bool tchain_possible(const uu3d_config& c) {
    return c.precision == UU3D_PREC_F16X3 && c.d_temporal == 384 && c.h_temporal == 768 && c.num_heads == 8 && c.temporal_depth >= 1;
}

int fail(uu3d_model* m, int code, const std::string& msg) {
    if (m) m->err = msg; else g_create_error = msg;
    return code;
}

#define HIPCHK(m, expr)                                                                         \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess)                                                                  \
            return fail(m, UU3D_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));   \
    } while (0)

// The frames form of a handle with generic dims (include/uu3d.h, FRAMES FORM): the spatial stack of a frame runs in one workgroup
// (uu3d_spatial_generic.h), so the frame has to fit the CU's LDS.  One rule, asked by every entry point of the frames form before it
// launches anything; compiled dims always have the form.
inline bool has_frames_form(const uu3d_model* m) {
    const uu3d_config& c = m->cfg;
    return !m->generic || spatial_generic_lds_bytes(c.num_keypoints, c.d_spatial, c.h_spatial, c.num_heads) <= SG_LDS_LIMIT;
}
int no_frames_form(uu3d_model* m, const std::string& who) {
    const uu3d_config& c = m->cfg;
    return fail(m, UU3D_ERR_UNSUPPORTED, who + ": this handle with generic dims has no frames form: the spatial stack of one frame needs " +
                std::to_string(spatial_generic_lds_bytes(c.num_keypoints, c.d_spatial, c.h_spatial, c.num_heads)) + " bytes of LDS, a workgroup has " +
                std::to_string(SG_LDS_LIMIT) + " (the window forward is unaffected)");
}

void add_weight(uu3d_model* m, const std::string& name, std::vector<int64_t> dims) {
    WeightRec r;
    r.name = name;
    r.dims = dims;
    r.numel = 1;
    for (auto d : dims) r.numel *= d;
    m->index[name] = (int)m->weights.size();
    m->weights.push_back(std::move(r));
}

void add_block(uu3d_model* m, const std::string& p, int d, int h, bool strided, bool qkv_bias) {
    add_weight(m, p + "/norm1/gamma", {d});
    add_weight(m, p + "/norm1/beta", {d});
    for (const char* nm : {"wq", "wk", "wv"}) {
        add_weight(m, p + "/attn/" + nm + "/kernel", {d, d});
        if (qkv_bias) add_weight(m, p + "/attn/" + nm + "/bias", {d});
    }
    add_weight(m, p + "/attn/projection/kernel", {d, d});
    add_weight(m, p + "/attn/projection/bias", {d});
    add_weight(m, p + "/norm2/gamma", {d});
    add_weight(m, p + "/norm2/beta", {d});
    if (strided) {
        add_weight(m, p + "/mlp/fc1/kernel", {1, d, h});
        add_weight(m, p + "/mlp/fc1/bias", {h});
        add_weight(m, p + "/mlp/strided_conv/kernel", {3, h, d});
        add_weight(m, p + "/mlp/strided_conv/bias", {d});
    } else {
        add_weight(m, p + "/mlp/fc1/kernel", {d, h});
        add_weight(m, p + "/mlp/fc1/bias", {h});
        add_weight(m, p + "/mlp/fc2/kernel", {h, d});
        add_weight(m, p + "/mlp/fc2/bias", {d});
    }
}

// Creation order of the reference's __init__ (u_u_t.py:196-285) = model.weights order.
void build_inventory(uu3d_model* m) {
    const uu3d_config& c = m->cfg;
    const int J = c.num_keypoints, N = c.num_frames, ds = c.d_spatial, dt = c.d_temporal;
    if (c.spatial_depth > 0) {
        add_weight(m, "keypoint_embedding/kernel", {2, ds});
        add_weight(m, "keypoint_embedding/bias", {ds});
        add_weight(m, "spatial_pe/positional_encoding_weights", {J, ds});
    }
    add_weight(m, "temporal_pe/positional_encoding_weights", {N, dt});
    for (int i = 0; i < c.num_strided; ++i)
        add_weight(m, "strided_temporal_pe_" + std::to_string(i + 1) + "/positional_encoding_weights", {m->L[i], dt});
    if (c.learnable_masked_token) add_weight(m, "learnable_masked_token_layer/learnable_masked_token", {dt});      // (u_u_t.py:219-220, in front of the strided-input token)
    if (c.has_strided_input) add_weight(m, "strided_input_token_layer/learnable_masked_token", {dt});
    if (c.spatial_depth > 0) {
        for (int i = 0; i < c.spatial_depth; ++i)
            add_block(m, "spatial_block_" + std::to_string(i + 1), ds, c.h_spatial, false, c.qkv_bias != 0);
        add_weight(m, "spatial_norm/gamma", {ds});
        add_weight(m, "spatial_norm/beta", {ds});
    }
    add_weight(m, "spatial_to_temporal_fc/kernel", {(int64_t)J * ds, dt});
    add_weight(m, "spatial_to_temporal_fc/bias", {dt});
    for (int i = 0; i < c.temporal_depth; ++i)
        add_block(m, "temporal_block_" + std::to_string(i + 1), dt, c.h_temporal, false, c.qkv_bias != 0);
    for (int i = 0; i < c.num_strided; ++i)
        add_block(m, "strided_temporal_block_" + std::to_string(i + 1), dt, c.h_temporal, true, c.qkv_bias != 0);
    // Keras' model.weights = trainable weights in creation order, then the non-trainable ones (the BatchNorm moving statistics)
    if (c.full_output && c.temporal_depth > 0) {
        if (c.output_bn) { add_weight(m, "temporal_norm/gamma", {dt}); add_weight(m, "temporal_norm/beta", {dt}); }
        add_weight(m, "temporal_fc/kernel", {dt, 3 * J});
        add_weight(m, "temporal_fc/bias", {3 * J});
    }
    if (c.output_bn) { add_weight(m, "strided_temporal_norm/gamma", {dt}); add_weight(m, "strided_temporal_norm/beta", {dt}); }
    add_weight(m, "strided_temporal_fc/kernel", {dt, 3 * J});
    add_weight(m, "strided_temporal_fc/bias", {3 * J});
    if (c.output_bn) {
        if (c.full_output && c.temporal_depth > 0) { add_weight(m, "temporal_norm/moving_mean", {dt}); add_weight(m, "temporal_norm/moving_variance", {dt}); }
        add_weight(m, "strided_temporal_norm/moving_mean", {dt}); add_weight(m, "strided_temporal_norm/moving_variance", {dt});
    }
}

}  // namespace


// =========================================================================================
// Definitions below take C linkage from their extern "C" declarations in include/uu3d.h.

#ifdef UU3D_TIMING_BUILD
const char* uu3d_version(void) { return "uu3d 0.3.0 gfx950 f16x3+f32-mfma timing-build (UU3D_SKIP / UU3D_TIMING_PARTS honoured: results can be wrong)"; }
#else
const char* uu3d_version(void) { return "uu3d 0.3.0 gfx950 f16x3+f32-mfma"; }
#endif

const char* uu3d_status_string(int s) {
    switch (s) {
        case UU3D_OK: return "ok";
        case UU3D_ERR_INVALID_ARGUMENT: return "invalid argument";
        case UU3D_ERR_UNSUPPORTED: return "configuration not supported by the compiled kernels";
        case UU3D_ERR_SHAPE: return "shape mismatch";
        case UU3D_ERR_NOT_READY: return "weights not set/committed";
        case UU3D_ERR_WORKSPACE: return "workspace too small or misaligned";
        case UU3D_ERR_HIP: return "HIP runtime error";
        case UU3D_ERR_NO_DEVICE: return "no usable device";
        case UU3D_ERR_RANGE: return "values beyond the f16 range of the f16x3 products (or non-finite inputs)";
        default: return "unknown status";
    }
}

const char* uu3d_last_error(const uu3d_model* model) {
    return model ? model->err.c_str() : g_create_error.c_str();
}

int uu3d_create(const uu3d_config* c, int device, uu3d_model** out) {
    if (!c || !out) return fail(nullptr, UU3D_ERR_INVALID_ARGUMENT, "null config/out pointer");
    *out = nullptr;
    if (c->num_frames < 1 || c->num_keypoints < 1 || c->num_strided < 0 || c->num_strided > UU3D_MAX_STRIDED)
        return fail(nullptr, UU3D_ERR_INVALID_ARGUMENT, "bad num_frames/num_keypoints/num_strided");
    if (c->precision != UU3D_PREC_F32 && c->precision != UU3D_PREC_F16X3) return fail(nullptr, UU3D_ERR_UNSUPPORTED, "unknown precision");
    if (c->spatial_depth < 1) return fail(nullptr, UU3D_ERR_UNSUPPORTED, "spatial_depth must be >= 1");
    if (c->temporal_depth < 0) return fail(nullptr, UU3D_ERR_INVALID_ARGUMENT, "temporal_depth < 0");
    // the specialised kernels (all shipped configs): J = 17, d_s = 32, h_s = 64, 8 heads, d_t = 384.  Anything else the reference's constructor
    // accepts (SPATIAL_EMBED_DIM / TEMPORAL_EMBED_DIM / NUM_HEADS / MLP ratios, u_u_t_constructor.py:26-32) runs on the generic forward.
    const bool generic = c->num_keypoints != kJ || c->d_spatial != kDS || c->h_spatial != kHS || c->num_heads != kHeads || c->d_temporal != kDH * kHeads;
    if (generic) {
        if (c->num_heads < 1 || c->d_spatial < 1 || c->d_temporal < 1 || c->h_spatial < 1 || c->h_temporal < 1)
            return fail(nullptr, UU3D_ERR_INVALID_ARGUMENT, "dims and head count must be positive");
        if (c->d_spatial % c->num_heads != 0 || c->d_temporal % c->num_heads != 0)
            return fail(nullptr, UU3D_ERR_INVALID_ARGUMENT, "embed dims must be divisible by NUM_HEADS (vision_transformer.py:79)");
        if (!attn_generic_head_dim_ok(c->d_spatial / c->num_heads) || !attn_generic_head_dim_ok(c->d_temporal / c->num_heads))
            return fail(nullptr, UU3D_ERR_UNSUPPORTED, "generic forward: head dims (embed dim / NUM_HEADS) must be one of 2, 4, 8, 12, 16, 24, 32, 48, 64");
        if (c->d_spatial % 4 != 0 || c->d_temporal % 4 != 0 || c->h_spatial % 4 != 0)
            return fail(nullptr, UU3D_ERR_UNSUPPORTED, "generic forward: embed dims and MLP widths must be multiples of 4 (16-byte row pieces in every loader)");
        if (c->num_keypoints > 128 || c->num_frames > 128)
            return fail(nullptr, UU3D_ERR_UNSUPPORTED, "generic forward: at most 128 keypoints and 128 frames");
        if (c->temporal_depth < 1 || c->num_strided < 1 || !c->full_output)
            return fail(nullptr, UU3D_ERR_UNSUPPORTED, "generic forward: needs at least one temporal block, one strided block and the full-sequence head");
    }
    if (c->h_temporal % 4 != 0 || c->h_temporal < 4)
        return fail(nullptr, UU3D_ERR_UNSUPPORTED, "h_temporal must be a positive multiple of 4");
    // temporal_depth == 0 (u_u_t.py:356,372-380): the strided blocks follow the token blend directly and the FIRST one takes the key
    // mask; the reference hands the same (B, 1, 1, N) mask to every strided block below FIRST_STRIDED_TOKEN_ATTENTION_LAYER, which only
    // has the right shape for the first (N keys)
    if (c->temporal_depth == 0 && c->has_strided_input && c->num_strided > 0 && c->first_strided_token_attention_layer > 1)
        return fail(nullptr, UU3D_ERR_INVALID_ARGUMENT, "temporal_depth == 0 with FIRST_STRIDED_TOKEN_ATTENTION_LAYER > 1: the reference's key mask has N entries, strided block 2 has fewer keys");
    if (c->d_temporal > 64 * 4 * 4)
        return fail(nullptr, UU3D_ERR_UNSUPPORTED, "d_temporal > 1024");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return fail(nullptr, UU3D_ERR_NO_DEVICE, "HIP device not available");

    auto* m = new uu3d_model();
    m->cfg = *c;
    m->device = device;
    m->generic = generic;
    m->L.push_back(c->num_frames);
    for (int i = 0; i < c->num_strided; ++i) {
        if (c->strides[i] < 1 || c->pad_left[i] < 0 || c->pad_right[i] < 0) {
            delete m;
            return fail(nullptr, UU3D_ERR_INVALID_ARGUMENT, "bad stride/padding");
        }
        const int Lin = m->L.back();
        const int Lout = (Lin + c->pad_left[i] + c->pad_right[i] - 3) / c->strides[i] + 1;
        if (Lin + c->pad_left[i] + c->pad_right[i] < 3 || Lout < 1) {
            delete m;
            return fail(nullptr, UU3D_ERR_INVALID_ARGUMENT, "strided block reduces the sequence below one token");
        }
        // exact-f32 attention holds a query tile's logits in registers (<= 128 keys); the f16x3 kernel tiles the keys
        if (Lin > (c->precision == UU3D_PREC_F16X3 ? ATTN_H3_MAX_L : 128)) {
            delete m;
            return fail(nullptr, UU3D_ERR_UNSUPPORTED, c->precision == UU3D_PREC_F16X3 ? "sequence length > 416 tokens" : "sequence length > 128 tokens with precision f32");
        }
        m->L.push_back(Lout);
    }
    if (c->num_strided > 0 && m->L.back() != 1) {
        delete m;   // einops "b n (p c) -> (b n) p c", n=1 fails in the reference (u_u_t.py:416)
        return fail(nullptr, UU3D_ERR_INVALID_ARGUMENT, "STRIDES/PADDINGS must reduce the sequence to one token");
    }
    build_inventory(m);
    m->sw = read_switches();
    { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, device) == hipSuccess && pr.multiProcessorCount > 0) m->num_cus = pr.multiProcessorCount; }
    // (the handle's device, not the caller's current one: every later call of the library sets it as well)
    if (hipSetDevice(device) != hipSuccess) {
        delete m;
        return fail(nullptr, UU3D_ERR_HIP, "hipSetDevice failed");
    }
    if (hipMalloc((void**)&m->d_range, 2 * sizeof(int)) != hipSuccess || hipMemset(m->d_range, 0, 2 * sizeof(int)) != hipSuccess) {      // [0] the sticky word, [1] what uu3d_range_status took
        delete m;
        return fail(nullptr, UU3D_ERR_HIP, "hipMalloc of the range-guard word failed");
    }
    *out = m;
    return UU3D_OK;
}

static void train_free(uu3d_model* m);
static int generic_forward(uu3d_model* m, const float* kp2d, const uint8_t* mask, int32_t B, float* full_out, float* central_out,
                           float* const* attn_out, void* workspace, size_t workspace_bytes, void* stream);      // uu3d_train_entry.inc
namespace { struct FramesIn; }
static int generic_forward_frames(uu3d_model* m, const FramesIn& frames, const uint8_t* mask, int32_t B, float* full_out, float* central_out,
                                  float* const* attn_out, void* workspace, size_t workspace_bytes, void* stream);   // uu3d_train_entry.inc
static size_t generic_frame_features_bytes(const uu3d_model* m, long F);                                                // uu3d_train_entry.inc
static int generic_frame_features(uu3d_model* m, const float* frames_dev, int32_t F, float* features, void* workspace, size_t workspace_bytes,
                                  void* stream);                                                                        // uu3d_train_entry.inc
static int generic_op_spatial_stack(uu3d_model* m, const float* frames_dev, int32_t F, float* S, void* stream);         // uu3d_train_entry.inc
void uu3d_destroy(uu3d_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    train_free(m);
    if (m->gparams) (void)hipFree(m->gparams);
    if (m->arena) (void)hipFree(m->arena);
    if (m->harena) (void)hipFree(m->harena);
    if (m->d_range) (void)hipFree(m->d_range);
    for (auto& r : m->prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    delete m;
}

int uu3d_num_weights(const uu3d_model* m) { return m ? (int)m->weights.size() : 0; }

int uu3d_weight_info(const uu3d_model* m, int i, const char** name, int32_t* ndim, int64_t dims[4]) {
    if (!m || i < 0 || i >= (int)m->weights.size()) return UU3D_ERR_INVALID_ARGUMENT;
    const WeightRec& r = m->weights[i];
    if (name) *name = r.name.c_str();
    if (ndim) *ndim = (int32_t)r.dims.size();
    if (dims) for (size_t k = 0; k < 4; ++k) dims[k] = k < r.dims.size() ? r.dims[k] : 1;
    return UU3D_OK;
}

int uu3d_set_weight(uu3d_model* m, const char* name, const float* data, int64_t numel) {
    if (!m || !name || !data) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "null argument to uu3d_set_weight");
    auto it = m->index.find(name);
    if (it == m->index.end()) return fail(m, UU3D_ERR_INVALID_ARGUMENT, std::string("unknown weight: ") + name);
    WeightRec& r = m->weights[it->second];
    if (numel != r.numel)
        return fail(m, UU3D_ERR_SHAPE, std::string("element count mismatch for ") + name + ": got " +
                                           std::to_string(numel) + ", expected " + std::to_string(r.numel));
    r.host.assign(data, data + numel);
    r.set = true;
    m->committed = false;
    return UU3D_OK;
}

int uu3d_get_weight(const uu3d_model* mc, const char* name, float* out, int64_t numel) {
    auto* m = const_cast<uu3d_model*>(mc);
    if (!m || !name || !out) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "null argument to uu3d_get_weight");
    auto it = m->index.find(name);
    if (it == m->index.end()) return fail(m, UU3D_ERR_INVALID_ARGUMENT, std::string("unknown weight: ") + name);
    const WeightRec& r = m->weights[it->second];
    if (!r.set) return fail(m, UU3D_ERR_NOT_READY, std::string("weight never set: ") + name);
    if (numel != r.numel) return fail(m, UU3D_ERR_SHAPE, std::string("element count mismatch for ") + name);
    std::memcpy(out, r.host.data(), sizeof(float) * (size_t)numel);
    return UU3D_OK;
}

#include "uu3d_commit.inc"
#include "uu3d_forward.inc"

int uu3d_range_status(uu3d_model* m, void* stream, int32_t* out_flag) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    HIPCHK(m, hipSetDevice(m->device));
    int h = 0;
    hipLaunchKernelGGL(range_take_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, m->d_range, m->d_range + 1);      // read and clear: ONE atomic exchange
    HIPCHK(m, hipMemcpyAsync(&h, m->d_range + 1, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(m, hipStreamSynchronize((hipStream_t)stream));
    if (out_flag) *out_flag = h != 0;
    if (h != 0) return fail(m, UU3D_ERR_RANGE, "non-finite values in a forward's outputs: activations beyond the f16 range (65504) of the f16x3 products, or non-finite inputs "
                                               "(repeat the batch with UU3D_SCHEDULE_EXACT_F32 or build the model with precision f32)");
    return UU3D_OK;
}

int uu3d_mpjpe(const float* pred, const float* gt, int32_t B, int32_t J, int32_t root, double* out, void* stream) {
    if (!pred || !gt || !out || B < 1 || J < 1 || root < 0 || root >= J) return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(mpjpe_kernel, dim3((B * J + 255) / 256), dim3(256), 0, (hipStream_t)stream, pred, gt, B, J, root, out);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

// ---- evaluation report on the device (uu3d_metrics.h) ----
size_t uu3d_error_sums_scratch_bytes(int64_t num_poses, int32_t num_actions) {
    if (num_poses < 1 || num_actions < 0 || num_actions > kMetMaxActions) return 0;
    return (size_t)kMetMaxGrid * (size_t)(num_actions + 1) * 6 * sizeof(double);
}

static bool met_sums_args_ok(int64_t P, const int32_t* actions, int32_t A, double* sums, void* scratch, size_t scratch_bytes) {
    if (A < 0 || A > kMetMaxActions || (A > 0 && !actions) || !sums || !scratch || ((uintptr_t)scratch & 7) != 0) return false;
    return scratch_bytes >= uu3d_error_sums_scratch_bytes(P, A);
}

int uu3d_pose_errors(const void* pred, int64_t R, const int32_t* left, const int32_t* right, const double* weight, const void* gt,
                     int64_t P, int32_t J, int32_t Cg, int32_t root, int32_t inputs_f64, double* errors, const int32_t* actions,
                     int32_t A, const uint8_t* select, double* sums, void* scratch, size_t scratch_bytes, void* stream_) {
    if (!pred || !gt || R < 1 || P < 1 || J < 1 || J > kMetMaxJoints || (Cg != 3 && Cg != 4) || root < 0 || root >= J ||
        (inputs_f64 != 0 && inputs_f64 != 1) || (!errors && !sums) || (weight && (!left || !right)) || (!left && P > R) ||
        P > (int64_t)1 << 40 || R > INT32_MAX)
        return UU3D_ERR_INVALID_ARGUMENT;
    if (sums && !met_sums_args_ok(P, actions, A, sums, scratch, scratch_bytes)) return UU3D_ERR_INVALID_ARGUMENT;
    hipStream_t stream = (hipStream_t)stream_;
    const int elem = inputs_f64 ? 8 : 4;
    const int gstride = (J * Cg) | 1;
    const int per_pose = ((J * 3) | 1) * 8 + gstride * elem;
    const int ppb = std::min(kMetLanes, kMetLdsBudget / per_pose);
    const long tiles = (P + ppb - 1) / ppb;
    const int grid = (int)std::min<long>(tiles, kMetMaxGrid);
    double* partial = sums ? (double*)scratch : nullptr;
    if (inputs_f64)
        hipLaunchKernelGGL(pose_errors_kernel<double>, dim3(grid), dim3(kMetLanes), (size_t)ppb * per_pose, stream, (const double*)pred, (long)R, left,
                           right, weight, (const double*)gt, (long)P, J, Cg, root, ppb, gstride, errors, actions, A, select, partial);
    else
        hipLaunchKernelGGL(pose_errors_kernel<float>, dim3(grid), dim3(kMetLanes), (size_t)ppb * per_pose, stream, (const float*)pred, (long)R, left,
                           right, weight, (const float*)gt, (long)P, J, Cg, root, ppb, gstride, errors, actions, A, select, partial);
    if (hipGetLastError() != hipSuccess) return UU3D_ERR_HIP;
    if (sums) {
        hipLaunchKernelGGL(error_sums_combine_kernel, dim3(1), dim3(64), 0, stream, partial, grid, (A + 1) * 6, sums);
        if (hipGetLastError() != hipSuccess) return UU3D_ERR_HIP;
    }
    return UU3D_OK;
}

int uu3d_error_sums(const double* errors, int64_t P, int32_t J, const int32_t* actions, int32_t A, const uint8_t* select, double* sums,
                    void* scratch, size_t scratch_bytes, void* stream_) {
    if (!errors || P < 1 || P > (int64_t)1 << 40 || J < 1 || !met_sums_args_ok(P, actions, A, sums, scratch, scratch_bytes))
        return UU3D_ERR_INVALID_ARGUMENT;
    hipStream_t stream = (hipStream_t)stream_;
    const long tiles = (P + kMetLanes - 1) / kMetLanes;
    const int grid = (int)std::min<long>(tiles, kMetMaxGrid);
    hipLaunchKernelGGL(error_sums_kernel, dim3(grid), dim3(kMetLanes), 0, stream, errors, (long)P, J, actions, A, select, (double*)scratch);
    if (hipGetLastError() != hipSuccess) return UU3D_ERR_HIP;
    hipLaunchKernelGGL(error_sums_combine_kernel, dim3(1), dim3(64), 0, stream, (const double*)scratch, grid, (A + 1) * 6, sums);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_gather_windows_valid(const float* poses, const int64_t* video_start, const int32_t* video_len, const uu3d_window* windows,
                              const int32_t* flip_order, int32_t B, int32_t N, int32_t J, int32_t Cc, int32_t pad_edge,
                              int32_t zero_masked, const uint8_t* frame_valid, float* out, uint8_t* stride_mask, uint8_t* pad_mask, void* stream) {
    if (!poses || !video_start || !video_len || !windows || !out || !stride_mask || B < 1 || N < 1 || J < 1 || Cc < 1 || Cc > 4)
        return UU3D_ERR_INVALID_ARGUMENT;
    static_assert(sizeof(uu3d_window) == sizeof(WindowDesc), "descriptor layouts must agree");
    const long total = (long)B * N * J;
    hipLaunchKernelGGL(gather_windows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       poses, video_start, video_len, reinterpret_cast<const WindowDesc*>(windows), flip_order,
                       B, N, J, Cc, pad_edge, zero_masked, frame_valid, out, stride_mask, pad_mask);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_gather_windows(const float* poses, const int64_t* video_start, const int32_t* video_len, const uu3d_window* windows,
                        const int32_t* flip_order, int32_t B, int32_t N, int32_t J, int32_t Cc, int32_t pad_edge,
                        int32_t zero_masked, float* out, uint8_t* stride_mask, uint8_t* pad_mask, void* stream) {
    return uu3d_gather_windows_valid(poses, video_start, video_len, windows, flip_order, B, N, J, Cc, pad_edge, zero_masked, nullptr, out,
                                     stride_mask, pad_mask, stream);
}

int uu3d_gather_window_frames_valid(const int64_t* video_start, const int32_t* video_len, const uu3d_window* windows, int32_t B, int32_t N,
                                    int32_t pad_edge, int32_t zero_masked, int64_t frame_base, int64_t zero_row, const uint8_t* frame_valid,
                                    int32_t* rows, uint8_t* stride_mask, uint8_t* pad_mask, void* stream) {
    if (!video_start || !video_len || !windows || !rows || !stride_mask || B < 1 || N < 1 || frame_base < 0 || zero_row < 0 || zero_row > INT32_MAX)
        return UU3D_ERR_INVALID_ARGUMENT;
    const long total = (long)B * N;
    hipLaunchKernelGGL(gather_window_frames_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       video_start, video_len, reinterpret_cast<const WindowDesc*>(windows), B, N, pad_edge, zero_masked,
                       frame_base, zero_row, frame_valid, rows, stride_mask, pad_mask);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_gather_window_frames(const int64_t* video_start, const int32_t* video_len, const uu3d_window* windows, int32_t B, int32_t N,
                              int32_t pad_edge, int32_t zero_masked, int64_t frame_base, int64_t zero_row, int32_t* rows,
                              uint8_t* stride_mask, uint8_t* pad_mask, void* stream) {
    return uu3d_gather_window_frames_valid(video_start, video_len, windows, B, N, pad_edge, zero_masked, frame_base, zero_row, nullptr, rows,
                                           stride_mask, pad_mask, stream);
}

namespace {
// uu3d_normalize_tracks (valid_out == nullptr: one launch) and uu3d_normalize_tracks_valid (the validity launch in front of it)
int normalize_tracks(const float* src, int64_t src_rows, float* table, int64_t rows, int32_t J, const int32_t* row_track, int32_t num_tracks,
                     const double* resolution, const int64_t* track_start, const int64_t* src_start, int32_t key_stride, const uint8_t* valid_in,
                     uint8_t* valid_out, void* stream) {
    if (!src || !table || !row_track || src_rows < 1 || rows < 1 || J < 1 || num_tracks < 1 || key_stride < 0) return UU3D_ERR_INVALID_ARGUMENT;
    if (key_stride > 0 && (!track_start || !src_start || src == table)) return UU3D_ERR_INVALID_ARGUMENT;
    if (key_stride == 0 && src_rows != rows) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)table & 15) != 0 || ((uintptr_t)src & 7) != 0) return UU3D_ERR_INVALID_ARGUMENT;
    if (valid_out != nullptr) {
        hipLaunchKernelGGL(track_valid_kernel, dim3((unsigned)(((long)rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                           src, (long)src_rows, (long)rows, J, row_track, num_tracks, track_start, src_start, key_stride, valid_in, valid_out);
        if (hipGetLastError() != hipSuccess) return UU3D_ERR_HIP;
    }
    const long threads = ((long)rows * J + 1) / 2;
    hipLaunchKernelGGL(normalize_tracks_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       src, (long)src_rows, table, (long)rows, J, row_track, num_tracks, resolution, track_start, src_start, key_stride,
                       (const uint8_t*)valid_out);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}
}  // namespace

int uu3d_normalize_tracks(const float* src, int64_t src_rows, float* table, int64_t rows, int32_t J, const int32_t* row_track, int32_t num_tracks,
                          const double* resolution, const int64_t* track_start, const int64_t* src_start, int32_t key_stride, void* stream) {
    return normalize_tracks(src, src_rows, table, rows, J, row_track, num_tracks, resolution, track_start, src_start, key_stride, nullptr, nullptr, stream);
}

int uu3d_normalize_tracks_valid(const float* src, int64_t src_rows, float* table, int64_t rows, int32_t J, const int32_t* row_track,
                                int32_t num_tracks, const double* resolution, const int64_t* track_start, const int64_t* src_start,
                                int32_t key_stride, const uint8_t* valid_in, uint8_t* valid_out, void* stream) {
    if (!valid_out) return UU3D_ERR_INVALID_ARGUMENT;
    return normalize_tracks(src, src_rows, table, rows, J, row_track, num_tracks, resolution, track_start, src_start, key_stride, valid_in, valid_out, stream);
}

int uu3d_resample_tracks(const float* src, int64_t src_rows, float* table, int64_t rows, int32_t J, const int32_t* row_track, int32_t num_tracks,
                         const double* resolution, const int64_t* left, const int64_t* right, const double* weight, const uint8_t* valid_in,
                         uint8_t* valid_out, void* stream) {
    if (!src || !table || !row_track || !left || !right || !weight || src_rows < 1 || rows < 1 || J < 1 || num_tracks < 1) return UU3D_ERR_INVALID_ARGUMENT;
    if (src == table || (valid_in != nullptr && valid_out == nullptr)) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)table & 15) != 0 || ((uintptr_t)src & 7) != 0) return UU3D_ERR_INVALID_ARGUMENT;
    if (src_rows > (INT64_MAX >> 4) / J || rows > (INT64_MAX >> 4) / J) return UU3D_ERR_INVALID_ARGUMENT;
    if (valid_out != nullptr) {
        hipLaunchKernelGGL(resample_valid_kernel, dim3((unsigned)(((long)rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                           src, (long)src_rows, (long)rows, J, row_track, num_tracks, left, right, valid_in, valid_out);
        if (hipGetLastError() != hipSuccess) return UU3D_ERR_HIP;
    }
    const long threads = ((long)rows * J + 1) / 2;
    hipLaunchKernelGGL(resample_tracks_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       src, (long)src_rows, table, (long)rows, J, row_track, num_tracks, resolution, left, right, weight, (const uint8_t*)valid_out);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

size_t uu3d_repair_joints_scratch_bytes(int64_t rows, int32_t J) {
    if (rows < 1 || rows > INT32_MAX || J < 1 || rows > (INT64_MAX >> 4) / J) return 0;
    return (size_t)rows * (size_t)J * 2 * sizeof(int32_t);
}

int uu3d_repair_joints(const float* src, int64_t rows, int32_t J, const uint8_t* joint_flags, const int64_t* track_start, int32_t num_tracks,
                       int32_t max_gap, float* out, uint8_t* frame_valid, uint8_t* joint_state, void* scratch, size_t scratch_bytes, void* stream) {
    if (!src || !track_start || !out || !frame_valid || !joint_state || !scratch || rows < 1 || J < 1 || num_tracks < 1 || max_gap < 1)
        return UU3D_ERR_INVALID_ARGUMENT;
    if (src == out) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)out & 15) != 0 || ((uintptr_t)src & 7) != 0 || ((uintptr_t)joint_state & 1) != 0 || ((uintptr_t)scratch & 3) != 0) return UU3D_ERR_INVALID_ARGUMENT;
    // rows index the plan as int32; rows * J and the grid of the plan launch (one workgroup per track and joint) stay in range
    if (rows > INT32_MAX || rows > (INT64_MAX >> 4) / J || (int64_t)num_tracks * J > INT32_MAX) return UU3D_ERR_INVALID_ARGUMENT;
    if (scratch_bytes < uu3d_repair_joints_scratch_bytes(rows, J)) return UU3D_ERR_INVALID_ARGUMENT;
    int32_t* left = static_cast<int32_t*>(scratch);
    int32_t* right = left + (long)rows * J;
    hipLaunchKernelGGL(repair_plan_kernel, dim3((unsigned)((long)num_tracks * J)), dim3(kRepairChunk), 0, (hipStream_t)stream,
                       src, joint_flags, (long)rows, J, track_start, left, right);
    if (hipGetLastError() != hipSuccess) return UU3D_ERR_HIP;
    const long threads = ((long)rows * J + 1) / 2;
    hipLaunchKernelGGL(repair_apply_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       src, joint_flags, (long)rows, J, (const int32_t*)left, (const int32_t*)right, max_gap, out, joint_state);
    if (hipGetLastError() != hipSuccess) return UU3D_ERR_HIP;
    hipLaunchKernelGGL(repair_flag_kernel, dim3((unsigned)(((long)rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t*)joint_state, (long)rows, J, frame_valid);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

// ---- ANY SKELETON (uu3d_keypoints.h): the table's size, its host-side packing, the one launch ----
size_t uu3d_keypoint_map_bytes(int32_t inputs, int32_t joints) {
    if (inputs < 1 || joints < 1 || joints > (1 << 20)) return 0;
    return keypoint_table_bytes(joints);
}

int uu3d_keypoint_map_pack(int32_t inputs, int32_t joints, const int32_t* counts, const int32_t* sources, const double* weights, void* out_host,
                           size_t out_bytes) {
    if (!counts || !sources || !weights || !out_host || ((uintptr_t)out_host & 7) != 0) return UU3D_ERR_INVALID_ARGUMENT;
    const size_t need = uu3d_keypoint_map_bytes(inputs, joints);
    if (need == 0 || out_bytes < need) return UU3D_ERR_INVALID_ARGUMENT;
    return keypoint_map_pack(inputs, joints, counts, sources, weights, out_host) == nullptr ? UU3D_OK : UU3D_ERR_INVALID_ARGUMENT;
}

int uu3d_map_keypoints(uu3d_model* m, const void* map, int32_t inputs, const float* src, const uint8_t* flags_in, int64_t frames, float* out,
                       uint8_t* flags_out, void* stream) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    const int J = m->cfg.num_keypoints;
    if (inputs < 1) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_map_keypoints: inputs must be >= 1");
    if ((flags_in == nullptr) != (flags_out == nullptr))
        return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_map_keypoints: flags_in_dev and flags_out_dev go together");
    if (frames < 0 || frames > (INT64_MAX >> 4) / J || frames > (INT64_MAX >> 4) / inputs || (frames * J + 255) / 256 > INT32_MAX)
        return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_map_keypoints: frames out of range");
    if (frames == 0) return UU3D_OK;
    if (!map || !src || !out || (const void*)src == (const void*)out)
        return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_map_keypoints: null buffer, or out_dev is src_dev");
    if (((uintptr_t)map & 7) != 0 || ((uintptr_t)src & 7) != 0 || ((uintptr_t)out & 7) != 0)
        return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_map_keypoints: map_dev, src_dev and out_dev must be 8-byte aligned");
    hipLaunchKernelGGL(map_keypoints_kernel, dim3((unsigned)((frames * J + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       keypoint_table(map, J), inputs, J, src, flags_in, (long)frames, out, flags_out);
    return hipGetLastError() == hipSuccess ? UU3D_OK : fail(m, UU3D_ERR_HIP, "uu3d_map_keypoints: launch failed");
}

// ---- ABSOLUTE ROOT POSITION (uu3d_root.h): the solve of every given frame, then the trajectory at the returned frames ----
int uu3d_solve_roots(const float* poses, const float* kp2d, const uint8_t* joint_flags, int64_t frames, int32_t J, const int32_t* row_track,
                     int32_t num_tracks, const double* cameras, int32_t min_joints, double* roots, uint8_t* solved, void* stream) {
    if (J > kRootMaxJoints) return UU3D_ERR_UNSUPPORTED;
    if (frames < 0 || J < 1 || num_tracks < 1 || min_joints < 2 || frames > (INT64_MAX >> 4) / J || (frames + 255) / 256 > INT32_MAX)
        return UU3D_ERR_INVALID_ARGUMENT;
    if (frames == 0) return UU3D_OK;
    if (!poses || !kp2d || !cameras || !roots || !solved) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)poses & 3) != 0 || ((uintptr_t)kp2d & 7) != 0 || ((uintptr_t)cameras & 7) != 0 || ((uintptr_t)roots & 7) != 0)
        return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(solve_roots_kernel, dim3((unsigned)((frames + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       poses, kp2d, joint_flags, (long)frames, J, row_track, num_tracks, cameras, min_joints, roots, solved);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

size_t uu3d_root_trajectory_scratch_bytes(int64_t frames) {
    if (frames < 1 || frames > INT32_MAX) return 0;
    return (size_t)frames * 2 * sizeof(int32_t);
}

int uu3d_root_trajectory(const double* roots, const uint8_t* solved, int64_t frames, const int64_t* track_start, int32_t num_tracks,
                         const int64_t* base, const int64_t* wnum, const int64_t* wden, int64_t out_frames, float* out_roots,
                         uint8_t* root_state, void* scratch, size_t scratch_bytes, void* stream) {
    if (!roots || !solved || !track_start || !base || !wnum || !wden || !out_roots || !root_state || !scratch || frames < 1 || num_tracks < 1 ||
        out_frames < 1)
        return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)roots & 7) != 0 || ((uintptr_t)out_roots & 3) != 0 || ((uintptr_t)scratch & 3) != 0) return UU3D_ERR_INVALID_ARGUMENT;
    // frames index the scans as int32; the grid of the last launch stays in range
    if (frames > INT32_MAX || (out_frames + 255) / 256 > INT32_MAX) return UU3D_ERR_INVALID_ARGUMENT;
    if (scratch_bytes < uu3d_root_trajectory_scratch_bytes(frames)) return UU3D_ERR_INVALID_ARGUMENT;
    int32_t* left = static_cast<int32_t*>(scratch);
    int32_t* right = left + (long)frames;
    hipLaunchKernelGGL(root_scan_kernel, dim3((unsigned)num_tracks), dim3(kRepairChunk), 0, (hipStream_t)stream,
                       solved, (long)frames, track_start, left, right);
    if (hipGetLastError() != hipSuccess) return UU3D_ERR_HIP;
    hipLaunchKernelGGL(root_trajectory_kernel, dim3((unsigned)((out_frames + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       roots, (long)frames, (const int32_t*)left, (const int32_t*)right, base, wnum, wden, (long)out_frames, out_roots, root_state);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

// ---- PER-FRAME DETECTIONS (uu3d_associate.h): the state block, its reset, whole videos, the one frame of a live tick ----
namespace {
// the settings of an association call: UU3D_OK, or what is wrong (capacities beyond 64: UU3D_ERR_UNSUPPORTED)
int associate_resolve(const uu3d_associate_params* a, AssocParams& p) {
    if (!a || a->slots < 1 || a->detections < 1 || a->keypoints < 1 || a->max_age < 0 || a->min_common < 1 || !(a->max_dist >= 0.0))
        return UU3D_ERR_INVALID_ARGUMENT;
    if (a->slots > kAssocMax || a->detections > kAssocMax || a->keypoints > kAssocMax) return UU3D_ERR_UNSUPPORTED;
    p = AssocParams{a->slots, a->detections, a->keypoints, a->max_age, a->min_common, a->max_dist * a->max_dist};
    return UU3D_OK;
}
}  // namespace

size_t uu3d_associate_state_bytes(int32_t slots, int32_t keypoints) {
    if (slots < 1 || slots > kAssocMax || keypoints < 1 || keypoints > kAssocMax) return 0;
    return assoc_layout(slots, keypoints).bytes;
}

int uu3d_associate_reset(const uu3d_associate_params* a, void* state, const uint8_t* slot_mask, void* stream) {
    AssocParams p;
    if (const int st = associate_resolve(a, p)) return st;
    if (!state || ((uintptr_t)state & 255) != 0) return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(associate_reset_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, p.S, p.K, (char*)state, slot_mask);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_associate_detections(const uu3d_associate_params* a, const float* dets, const int32_t* counts, const uint8_t* flags, int32_t flag_joints,
                              const int64_t* video_start, int32_t num_videos, int64_t frames, void* state, int32_t* assignment, int32_t* track_of,
                              int32_t* track_ids, uint8_t* born, uint8_t* alive, int32_t* counters, void* stream) {
    AssocParams p;
    if (const int st = associate_resolve(a, p)) return st;
    if (!dets || !video_start || !state || !assignment || !track_of || !counters || num_videos < 1 || num_videos > (1 << 20) || frames < 0 ||
        frames > ((int64_t)1 << 40))
        return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)dets & 7) != 0 || ((uintptr_t)state & 255) != 0) return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(associate_video_kernel, dim3((unsigned)num_videos), dim3(kAssocLanes), 0, (hipStream_t)stream, p, dets, counts, flags,
                       flag_joints != 0 ? 1 : 0, video_start, (long)frames, (char*)state, assignment, track_of, track_ids, born, alive, counters);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_stream_associate(const uu3d_associate_params* a, void* state, const float* dets, const int32_t* count, const uint8_t* flags,
                          int32_t flag_joints, float* kp_out, uint8_t* flags_out, int32_t flags_out_joints, uint8_t* active_out, uint8_t* born_out,
                          int32_t* assignment, int32_t* track_ids, int32_t* dropped, void* stream) {
    AssocParams p;
    if (const int st = associate_resolve(a, p)) return st;
    if (!state || !dets || !count || !kp_out || !flags_out || !active_out || !born_out || !assignment || !track_ids || !dropped)
        return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)dets & 7) != 0 || ((uintptr_t)kp_out & 7) != 0 || ((uintptr_t)state & 255) != 0 || (const void*)dets == (const void*)kp_out)
        return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(associate_step_kernel, dim3(1), dim3(kAssocLanes), 0, (hipStream_t)stream, p, (char*)state, dets, count, flags,
                       flag_joints != 0 ? 1 : 0, kp_out, flags_out, flags_out_joints != 0 ? 1 : 0, active_out, born_out, assignment, track_ids, dropped);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_assemble_tracks(const float* plain, const float* flipped, int64_t num_windows, const int32_t* flip_order, const int32_t* left,
                         const int32_t* right, const double* weight, int64_t num_frames, int32_t J, int32_t root_index, float* out, void* stream) {
    if (!plain || !left || !right || !weight || !out || num_windows < 1 || num_frames < 1 || J < 1 || root_index >= J) return UU3D_ERR_INVALID_ARGUMENT;
    if (flipped != nullptr && !flip_order) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)out & 15) != 0) return UU3D_ERR_INVALID_ARGUMENT;
    const long threads = ((long)num_frames * J * 3 + 3) / 4;
    hipLaunchKernelGGL(assemble_tracks_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       plain, flipped, (long)num_windows, flip_order, left, right, weight, (long)num_frames, J, root_index < 0 ? -1 : root_index, out);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_assemble_tracks_cubic(const float* plain, const float* flipped, int64_t num_windows, const int32_t* flip_order, const int32_t* before,
                               const int32_t* left, const int32_t* right, const int32_t* after, const double* weight, int64_t num_frames, int32_t J,
                               int32_t root_index, float* out, void* stream) {
    if (!plain || !before || !left || !right || !after || !weight || !out || num_windows < 1 || num_frames < 1 || J < 1 || root_index >= J)
        return UU3D_ERR_INVALID_ARGUMENT;
    if (flipped != nullptr && !flip_order) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)out & 15) != 0) return UU3D_ERR_INVALID_ARGUMENT;
    const long threads = ((long)num_frames * J * 3 + 3) / 4;
    hipLaunchKernelGGL(assemble_tracks_cubic_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       plain, flipped, (long)num_windows, flip_order, before, left, right, after, weight, (long)num_frames, J,
                       root_index < 0 ? -1 : root_index, out);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

#include "uu3d_stream_api.inc"
#include "uu3d_stream_drain_api.inc"
#include "uu3d_smooth_api.inc"
#include "uu3d_bones_api.inc"
#include "uu3d_rotations_api.inc"
#include "uu3d_undistort_api.inc"
#include "uu3d_world_api.inc"
#include "uu3d_views_api.inc"
#include "uu3d_view_match_api.inc"
#include "uu3d_view_align_api.inc"
#include "uu3d_triangulate_api.inc"
#include "uu3d_view_calibrate_api.inc"
#include "uu3d_lift_match_api.inc"
#include "uu3d_stream_views_api.inc"

int uu3d_world_to_cam_2d(const float* world, const float* cams, int32_t B, int32_t N, int32_t J, float* cam3d, float* kp2d, void* stream) {
    if (!world || !cams || B < 1 || N < 1 || J < 1 || (!cam3d && !kp2d)) return UU3D_ERR_INVALID_ARGUMENT;
    const long per = (long)N * J, total = per * B;
    hipLaunchKernelGGL(world_to_cam_2d_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, world, cams, per, total, cam3d, kp2d);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_set_schedule(uu3d_model* m, int32_t schedule) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    if (schedule != UU3D_SCHEDULE_LATENCY && schedule != UU3D_SCHEDULE_THROUGHPUT) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "unknown schedule");
    m->throughput = (schedule == UU3D_SCHEDULE_THROUGHPUT);
    return UU3D_OK;
}

int uu3d_set_profiling(uu3d_model* m, int32_t enabled) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    m->profiling = enabled != 0;
    m->prof_used = 0;
    return UU3D_OK;
}

int uu3d_profile_read(uu3d_model* m, uu3d_profile_entry* out, int32_t capacity, int32_t* count) {
    if (!m || !count) return UU3D_ERR_INVALID_ARGUMENT;
    *count = (int32_t)m->prof_used;
    if (!out) return UU3D_OK;
    for (size_t i = 0; i < m->prof_used && (int32_t)i < capacity; ++i) {
        ProfRec& r = m->prof[i];
        HIPCHK(m, hipEventSynchronize(r.e1));
        float ms = 0.f;
        HIPCHK(m, hipEventElapsedTime(&ms, r.e0, r.e1));
        uu3d_profile_entry& e = out[i];
        std::memset(&e, 0, sizeof e);
        std::snprintf(e.name, sizeof e.name, "%s", r.name.c_str());
        std::snprintf(e.kernel, sizeof e.kernel, "%s", r.kernel.c_str());
        e.ms = ms; e.flops = r.flops; e.bytes = r.bytes;
    }
    return UU3D_OK;
}


// ---- training-step arithmetic without back-propagation (T1, T3, T4) -----------------------------
int uu3d_mpjpe_loss(const float* pred_full, const float* pred_central, const float* gt3d, int32_t B, int32_t N,
                    int32_t J, int32_t root, float w_center, float w_seq, int32_t batch_size_norm, float* loss_out,
                    float* grad_full, float* grad_central, float* scratch, void* stream_) {
    if (!pred_central || !gt3d || !loss_out || !scratch || B < 1 || N < 1 || J < 1 || root < 0 || root >= J ||
        batch_size_norm < 1)
        return UU3D_ERR_INVALID_ARGUMENT;
    if ((long)B * N * J > (1L << 30)) return UU3D_ERR_INVALID_ARGUMENT;
    hipStream_t stream = (hipStream_t)stream_;
    const float norm_cen = (float)batch_size_norm * (float)J;
    const float norm_seq = (float)batch_size_norm * (float)N * (float)J;
    const bool has_seq = pred_full != nullptr;
    // d loss / d dist: w / norm (fallback without sequence loss: (w_c + w_s) / norm_cen)
    const float gs_cen = (has_seq ? w_center : (w_center + w_seq)) / norm_cen;
    const float gs_seq = w_seq / norm_seq;
    hipLaunchKernelGGL(mpjpe_loss_stage1, dim3(kLossGrid), dim3(256), 0, stream, pred_full, pred_central, gt3d, B, N, J,
                       root, gs_seq, gs_cen, has_seq ? grad_full : nullptr, grad_central, scratch);
    hipLaunchKernelGGL(mpjpe_loss_stage2, dim3(1), dim3(64), 0, stream, scratch, norm_seq, norm_cen, w_center, w_seq,
                       has_seq ? 1 : 0, loss_out);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_adamw_update(float* var, float* m, float* v, float* vhat, const float* grad, int64_t n, float lr, float wd, float beta1,
                      float beta2, float epsilon, int64_t step, void* stream) {
    return uu3d_adamw_update_guarded(var, m, v, vhat, grad, n, lr, wd, beta1, beta2, epsilon, step, nullptr, stream);
}

int uu3d_adamw_update_guarded(float* var, float* m, float* v, float* vhat, const float* grad, int64_t n, float lr, float wd, float beta1,
                              float beta2, float epsilon, int64_t step, const uint32_t* skip, void* stream) {
    if (!var || !m || !v || !grad || n < 1 || step < 1) return UU3D_ERR_INVALID_ARGUMENT;
    if ((((uintptr_t)var | (uintptr_t)m | (uintptr_t)v | (uintptr_t)vhat | (uintptr_t)grad) & 15) != 0) return UU3D_ERR_INVALID_ARGUMENT;
    // float32 like the TF kernel: alpha = lr * sqrt(1 - beta2^t) / (1 - beta1^t)
    // beta^t rounded once from double (libm powf and numpy's float32 power disagree by an ulp at some t, e.g. 0.9^4)
    const float b1p = (float)pow((double)beta1, (double)step), b2p = (float)pow((double)beta2, (double)step);
    const float alpha = lr * sqrtf(1.0f - b2p) / (1.0f - b1p);
    const long long n4 = n >> 2;
    const int grid = (int)std::min<long long>(std::max<long long>((n4 + 255) / 256, 1), 256 * 32);
    if (vhat) hipLaunchKernelGGL(adamw_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, var, m, v, vhat, grad, (long long)n, wd, alpha,
                                 1.0f - beta1, 1.0f - beta2, epsilon, skip);
    else hipLaunchKernelGGL(adamw_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, var, m, v, vhat, grad, (long long)n, wd, alpha,
                            1.0f - beta1, 1.0f - beta2, epsilon, skip);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_ema_update(float* ema, const float* w, int64_t n, float decay, void* stream) {
    if (!ema || !w || n < 1) return UU3D_ERR_INVALID_ARGUMENT;
    const int grid = (int)std::min<long long>((n + 255) / 256, 256 * 8);
    hipLaunchKernelGGL(ema_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, ema, w, (long long)n, 1.0f - decay);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

#include "uu3d_train_state.inc"
#include "uu3d_train_forward.inc"
#include "uu3d_train_backward.inc"
#include "uu3d_train_entry.inc"

