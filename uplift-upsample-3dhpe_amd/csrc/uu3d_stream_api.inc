// uu3d_stream_api.inc -- the host side of the live sessions (stream.StreamSession; include/uu3d.h, LIVE TRACKS), a piece of uu3d_api.hip: the
// plain session (uu3d_stream.h), a session with a frame rate and one with an output rate of its own (uu3d_stream_rate.h), and the roots
// of a session with a camera (uu3d_stream_root.h; no model: the conventions of uu3d_solve_roots).  Every entry point of a model is: null model, stream_resolve (one prologue, one order of checks), its own buffer checks, one launch, launched().
namespace {
// the session's settings checked against the model; nullptr = fine, else what is wrong
const char* stream_config_error(const uu3d_model* m, const uu3d_stream_config* s) {
    if (!s) return "null uu3d_stream_config";
    const uu3d_config& c = m->cfg;
    if (s->slots < 1 || s->slots > (1 << 20)) return "slots must be in [1, 2^20]";
    if (s->seq_stride < 1 || s->pred_stride < 1) return "seq_stride and pred_stride must be >= 1";
    if (s->mask_stride < s->seq_stride || s->mask_stride % s->seq_stride != 0) return "mask_stride must be a multiple of seq_stride";
    if (s->lookahead < 0 || (int64_t)s->lookahead > (int64_t)(c.num_frames / 2) * s->seq_stride) return "lookahead must be in [0, (num_frames / 2) * seq_stride]";
    if (s->root_index >= c.num_keypoints) return "root_index must be below num_keypoints (negative: absolute poses)";
    if ((int64_t)s->seq_stride * c.num_frames > (1 << 28)) return "seq_stride too large";
    const StreamLayout L = stream_layout(s->slots, c.num_frames, c.num_keypoints, c.d_temporal, s->seq_stride, s->mask_stride, s->lookahead, s->flip);
    if (L.table_rows > INT32_MAX / 2 || (int64_t)L.halves * s->slots * c.num_frames > INT32_MAX / 2) return "slots x ring capacity too large";
    return nullptr;
}
const char* stream_rate_error(const uu3d_stream_rate* r) {
    if (!r) return "null uu3d_stream_rate";
    if (r->a < 1 || r->a >= (1 << 20) || r->b < 1 || r->b >= (1 << 20)) return "a and b must be in [1, 2^20)";
    if (r->lookahead < 0 || r->lookahead > (1 << 24)) return "the source lookahead must be in [0, 2^24]";
    if (r->key_ring < 1 || r->key_ring > 4096) return "key_ring must be in [1, 4096]";
    return nullptr;
}
const char* stream_out_error(const uu3d_stream_out* o) {
    if (!o) return "null uu3d_stream_out";
    if (o->c < 1 || o->c >= (1 << 20) || o->d < 1 || o->d >= (1 << 20)) return "c and d must be in [1, 2^20)";
    if (o->pos_num < 1 || o->pos_num >= (1 << 20) || o->pos_den < 1 || o->pos_den >= (1 << 20)) return "pos_num and pos_den must be in [1, 2^20)";
    if (o->max_out < 1 || o->max_out > 64 || (long)o->max_out * o->d < o->c) return "max_out must be in [ceil(c / d), 64]";
    return nullptr;
}

// What a stream entry point works on: R and rate are set where the call has a rate, out where it has an output rate; base is the state
// block (checked only with kStreamState).
struct StreamCall { StreamLayout L; RateLayout R; RateParams rate; OutParams out; char* base; };
enum : int { kStreamRate = 1, kStreamState = 2, kStreamOut = 4 };   // the arguments an entry point takes besides the model and the settings

// The one prologue of the stream entry points, behind their null-model test: the settings against the model, then -- where the entry
// point takes them (`parts`) -- the rate, the state block, the output rate, checked in this order; then the layouts and kernel parameters.
int stream_resolve(uu3d_model* m, const uu3d_stream_config* s, const uu3d_stream_rate* r, const uu3d_stream_out* o, const void* state,
                   const int parts, const char* who, StreamCall& c) {
    if (!has_frames_form(m)) return no_frames_form(m, who);
    if (const char* e = stream_config_error(m, s)) return fail(m, UU3D_ERR_INVALID_ARGUMENT, std::string(who) + ": " + e);
    if (parts & kStreamRate) if (const char* e = stream_rate_error(r)) return fail(m, UU3D_ERR_INVALID_ARGUMENT, std::string(who) + ": " + e);
    if ((parts & kStreamState) && (!state || ((uintptr_t)state & 255) != 0))
        return fail(m, UU3D_ERR_INVALID_ARGUMENT, std::string(who) + ": state must be a 256-byte aligned block");
    if (parts & kStreamOut) if (const char* e = stream_out_error(o)) return fail(m, UU3D_ERR_INVALID_ARGUMENT, std::string(who) + ": " + e);
    const uu3d_config& mc = m->cfg;
    c = StreamCall{};
    c.L = stream_layout(s->slots, mc.num_frames, mc.num_keypoints, mc.d_temporal, s->seq_stride, s->mask_stride, s->lookahead, s->flip);
    c.base = (char*)const_cast<void*>(state);
    if (parts & kStreamRate) {
        c.R = rate_layout(c.L, mc.num_keypoints, r->key_ring);
        RateParams& p = c.rate;
        p.slots = s->slots; p.J = mc.num_keypoints; p.halves = c.L.halves; p.per_pose = c.L.per_pose; p.a = r->a; p.b = r->b;
        p.lookahead = r->lookahead; p.model_lookahead = s->lookahead; p.pred_stride = s->pred_stride; p.key_ring = c.R.key_ring; p.key_stride = c.R.key_stride;
    }
    if (parts & kStreamOut) c.out = OutParams{o->c, o->d, o->pos_num, o->pos_den, o->max_out};
    return UU3D_OK;
}
// behind a launch
int launched(uu3d_model* m, const char* who) {
    return hipGetLastError() == hipSuccess ? UU3D_OK : fail(m, UU3D_ERR_HIP, std::string(who) + ": launch failed");
}
// MISSED DETECTIONS need the masked token: a model without strided input has none
int stream_valid_check(uu3d_model* m, const char* who) {
    if (!m->cfg.has_strided_input) return fail(m, UU3D_ERR_UNSUPPORTED, std::string(who) + ": frame validity needs a model with strided input (the masked token)");
    return UU3D_OK;
}
dim3 blocks_of(const long threads) { return dim3((unsigned)((threads + 255) / 256)); }
}  // namespace

// ---- the plain session (uu3d_stream.h): the state block and the four launches around uu3d_frame_features / uu3d_forward_frames_ex ----
int uu3d_stream_state_layout(const uu3d_model* mc, const uu3d_stream_config* s, uu3d_stream_layout* out) {
    auto* m = const_cast<uu3d_model*>(mc);
    if (!m || !out) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c;
    if (const int st = stream_resolve(m, s, nullptr, nullptr, nullptr, 0, "uu3d_stream_state_layout", c)) return st;
    const StreamLayout& L = c.L;
    out->ring_capacity = L.cap; out->table_rows = L.table_rows; out->zero_row = L.zero_row;
    out->frames_offset = (int64_t)L.off_frames; out->held_offset = (int64_t)L.off_held; out->table_offset = (int64_t)L.off_table;
    out->bytes = (int64_t)L.bytes;
    return UU3D_OK;
}

size_t uu3d_stream_state_bytes(const uu3d_model* m, const uu3d_stream_config* s) {
    uu3d_stream_layout l;
    return uu3d_stream_state_layout(m, s, &l) == UU3D_OK ? (size_t)l.bytes : 0;
}

size_t uu3d_stream_valid_bytes(const uu3d_model* mc, const uu3d_stream_config* s) {
    auto* m = const_cast<uu3d_model*>(mc);
    StreamCall c;
    if (!m || stream_resolve(m, s, nullptr, nullptr, nullptr, 0, "uu3d_stream_valid_bytes", c) != UU3D_OK) return 0;
    return (size_t)s->slots * (size_t)(c.L.cap + 1);
}

namespace {
// uu3d_stream_stage (valid_in == valid_out == nullptr) and uu3d_stream_stage_valid, behind their checks of the settings
int stream_stage(uu3d_model* m, const uu3d_stream_config* s, const float* kp, const double* resolution, const uint8_t* active,
                 const int32_t* flip_order, const uint8_t* valid_in, uint8_t* valid_out, float* frames_out, void* stream) {
    if (!kp || !active || !frames_out || (s->flip && !flip_order)) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_stage: null buffer");
    if (((uintptr_t)frames_out & 15) != 0 || ((uintptr_t)kp & 7) != 0) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_stage: frames_out must be 16-byte, kp 8-byte aligned");
    const int halves = s->flip ? 2 : 1;
    hipLaunchKernelGGL(stream_stage_kernel, blocks_of(((long)halves * s->slots * m->cfg.num_keypoints + 1) / 2), dim3(256), 0, (hipStream_t)stream,
                       kp, resolution, active, flip_order, s->slots, m->cfg.num_keypoints, halves, valid_in, valid_out, frames_out);
    return launched(m, "uu3d_stream_stage");
}
// what the commit kernels need to know about the session
StreamParams stream_params(const uu3d_model* m, const uu3d_stream_config* s, const StreamLayout& L) {
    StreamParams p{};
    p.slots = s->slots; p.N = m->cfg.num_frames; p.dt = m->cfg.d_temporal; p.seq_stride = s->seq_stride; p.s_in = s->mask_stride;
    p.pred_stride = s->pred_stride; p.lookahead = s->lookahead; p.cap = L.cap; p.halves = L.halves; p.pad_edge = s->pad_edge != 0;
    p.zero_row = (int)L.zero_row;
    p.masked_row = m->cfg.has_strided_input ? -1 : (int)L.zero_row;      // (no strided input: a dropped frame is read as zeros, eval.py:67)
    return p;
}
// uu3d_stream_commit (valid == valid_state == nullptr) and uu3d_stream_commit_valid
int stream_commit(uu3d_model* m, const uu3d_stream_config* s, const StreamCall& c, const float* features, const uint8_t* active, const uint8_t* valid,
                  uint8_t* valid_state, int32_t* rows, uint8_t* stride_mask, uint8_t* fresh, void* stream) {
    if (!c.base || !features || !active || !rows || !stride_mask || !fresh) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_commit: null buffer");
    if (((uintptr_t)c.base & 255) != 0 || ((uintptr_t)features & 15) != 0) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_commit: state must be 256-byte, features 16-byte aligned");
    const StreamLayout& L = c.L;
    const StreamParams p = stream_params(m, s, L);
    hipLaunchKernelGGL(stream_commit_kernel, dim3(s->slots), dim3(256), 0, (hipStream_t)stream, p, features, active,
                       (int32_t*)(c.base + L.off_frames), (float*)(c.base + L.off_table), rows, stride_mask, fresh, valid, valid_state);
    return launched(m, "uu3d_stream_commit");
}
}  // namespace

int uu3d_stream_stage(uu3d_model* m, const uu3d_stream_config* s, const float* kp, const double* resolution, const uint8_t* active,
                      const int32_t* flip_order, float* frames_out, void* stream) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c;
    if (const int st = stream_resolve(m, s, nullptr, nullptr, nullptr, 0, "uu3d_stream_stage", c)) return st;
    return stream_stage(m, s, kp, resolution, active, flip_order, nullptr, nullptr, frames_out, stream);
}

int uu3d_stream_stage_valid(uu3d_model* m, const uu3d_stream_config* s, const float* kp, const double* resolution, const uint8_t* active,
                            const int32_t* flip_order, const uint8_t* valid_in, uint8_t* valid_out, float* frames_out, void* stream) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c;
    if (const int st = stream_resolve(m, s, nullptr, nullptr, nullptr, 0, "uu3d_stream_stage_valid", c)) return st;
    if (const int st = stream_valid_check(m, "uu3d_stream_stage_valid")) return st;
    if (!valid_out) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_stage_valid: null valid_out");
    return stream_stage(m, s, kp, resolution, active, flip_order, valid_in, valid_out, frames_out, stream);
}

int uu3d_stream_commit(uu3d_model* m, const uu3d_stream_config* s, void* state, const float* features, const uint8_t* active,
                       int32_t* rows, uint8_t* stride_mask, uint8_t* fresh, void* stream) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c;
    if (const int st = stream_resolve(m, s, nullptr, nullptr, state, 0, "uu3d_stream_commit", c)) return st;
    return stream_commit(m, s, c, features, active, nullptr, nullptr, rows, stride_mask, fresh, stream);
}

int uu3d_stream_commit_valid(uu3d_model* m, const uu3d_stream_config* s, void* state, const float* features, const uint8_t* active,
                             const uint8_t* valid, void* valid_state, int32_t* rows, uint8_t* stride_mask, uint8_t* fresh, void* stream) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c;
    if (const int st = stream_resolve(m, s, nullptr, nullptr, state, 0, "uu3d_stream_commit_valid", c)) return st;
    if (const int st = stream_valid_check(m, "uu3d_stream_commit_valid")) return st;
    if (!valid || !valid_state) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_commit_valid: null validity buffer");
    return stream_commit(m, s, c, features, active, valid, (uint8_t*)valid_state, rows, stride_mask, fresh, stream);
}

int uu3d_stream_emit(uu3d_model* m, const uu3d_stream_config* s, void* state, const float* central, const int32_t* flip_order,
                     const uint8_t* fresh, float* out, void* stream) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c;
    if (const int st = stream_resolve(m, s, nullptr, nullptr, state, 0, "uu3d_stream_emit", c)) return st;
    if (!state || !central || !fresh || !out || (s->flip && !flip_order)) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_emit: null buffer");
    if (((uintptr_t)state & 255) != 0 || ((uintptr_t)out & 15) != 0) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_emit: state must be 256-byte, out 16-byte aligned");
    hipLaunchKernelGGL(stream_emit_kernel, blocks_of(((long)s->slots * c.L.per_pose + 3) / 4), dim3(256), 0, (hipStream_t)stream, central, c.L.halves,
                       flip_order, fresh, s->slots, m->cfg.num_keypoints, s->root_index < 0 ? -1 : s->root_index,
                       (float*)(c.base + c.L.off_held), out);
    return launched(m, "uu3d_stream_emit");
}

int uu3d_stream_reset(uu3d_model* m, const uu3d_stream_config* s, void* state, const uint8_t* slot_mask, void* stream) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c;
    if (const int st = stream_resolve(m, s, nullptr, nullptr, state, kStreamState, "uu3d_stream_reset", c)) return st;
    hipLaunchKernelGGL(stream_reset_kernel, blocks_of((long)s->slots * c.L.per_pose), dim3(256), 0, (hipStream_t)stream, slot_mask, s->slots,
                       c.L.per_pose, (int32_t*)(c.base + c.L.off_frames), (float*)(c.base + c.L.off_held));
    return launched(m, "uu3d_stream_reset");
}

// ---- live per-joint missed detections (uu3d_stream_repair.h): the repair state and the two launches that replace stage and commit ----
namespace {
// max_gap and the model behind stream_resolve -> the layout of the repair state and the stage kernel's parameters
int stream_repair_resolve(uu3d_model* m, const uu3d_stream_config* s, const int32_t max_gap, const char* who, StreamCall& c, RepairLayout& R, RepairParams& p) {
    if (const int st = stream_resolve(m, s, nullptr, nullptr, nullptr, 0, who, c)) return st;
    if (const int st = stream_valid_check(m, who)) return st;
    if (max_gap < 1 || max_gap > kLiveRepairMaxGap) return fail(m, UU3D_ERR_INVALID_ARGUMENT, std::string(who) + ": max_gap must be in [1, 32]");
    R = repair_layout(s->slots, m->cfg.num_keypoints, s->mask_stride, max_gap);
    if ((int64_t)c.L.halves * s->slots * R.K > INT32_MAX / 2) return fail(m, UU3D_ERR_INVALID_ARGUMENT, std::string(who) + ": slots x staged frames too large");
    p = RepairParams{s->slots, m->cfg.num_keypoints, max_gap, R.W, R.K, s->mask_stride, s->seq_stride, c.L.halves};
    return UU3D_OK;
}
}  // namespace

int uu3d_stream_repair_layout(const uu3d_model* mc, const uu3d_stream_config* s, int32_t max_gap, uu3d_stream_repair_state_layout* out) {
    auto* m = const_cast<uu3d_model*>(mc);
    if (!m || !out) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c; RepairLayout R; RepairParams p;
    if (const int st = stream_repair_resolve(m, s, max_gap, "uu3d_stream_repair_layout", c, R, p)) return st;
    out->window = R.W; out->staged_frames = R.K; out->raw_offset = (int64_t)R.off_raw; out->last_xy_offset = (int64_t)R.off_last_xy;
    out->last_offset = (int64_t)R.off_last; out->held_offset = (int64_t)R.off_held; out->observed_offset = (int64_t)R.off_observed;
    out->bytes = (int64_t)R.bytes;
    return UU3D_OK;
}

size_t uu3d_stream_repair_bytes(const uu3d_model* m, const uu3d_stream_config* s, int32_t max_gap) {
    uu3d_stream_repair_state_layout l;
    return uu3d_stream_repair_layout(m, s, max_gap, &l) == UU3D_OK ? (size_t)l.bytes : 0;
}

int uu3d_stream_repair_stage(uu3d_model* m, const uu3d_stream_config* s, int32_t max_gap, const void* state, void* repair_state, const float* kp,
                             const double* resolution, const uint8_t* active, const int32_t* flip_order, const uint8_t* joint_flags,
                             float* frames_out, int32_t* stage_frame, uint8_t* stage_valid, int32_t* far_frames, uint8_t* joint_state, void* stream) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c; RepairLayout R; RepairParams p;
    if (const int st = stream_repair_resolve(m, s, max_gap, "uu3d_stream_repair_stage", c, R, p)) return st;
    if (!state || !repair_state || !kp || !active || !frames_out || !stage_frame || !stage_valid || !far_frames || !joint_state || (s->flip && !flip_order))
        return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_repair_stage: null buffer");
    if (((uintptr_t)state & 255) != 0 || ((uintptr_t)repair_state & 255) != 0 || ((uintptr_t)frames_out & 15) != 0 || ((uintptr_t)kp & 7) != 0)
        return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_repair_stage: state and repair_state must be 256-byte, frames_out 16-byte, kp 8-byte aligned");
    char* rb = (char*)repair_state;
    hipLaunchKernelGGL(stream_repair_stage_kernel, dim3(s->slots), dim3(64), 0, (hipStream_t)stream, p, kp, resolution, active, flip_order, joint_flags,
                       (const int32_t*)((const char*)state + c.L.off_frames), (float*)(rb + R.off_raw), (float*)(rb + R.off_last_xy),
                       (int32_t*)(rb + R.off_last), (uint32_t*)(rb + R.off_held), (uint8_t*)(rb + R.off_observed), frames_out, stage_frame,
                       stage_valid, far_frames, joint_state);
    return launched(m, "uu3d_stream_repair_stage");
}

int uu3d_stream_commit_repair(uu3d_model* m, const uu3d_stream_config* s, int32_t max_gap, void* state, const float* features, const uint8_t* active,
                              const int32_t* stage_frame, const uint8_t* stage_valid, const int32_t* far_frames, void* valid_state, int32_t* rows,
                              uint8_t* stride_mask, uint8_t* fresh, void* stream) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c; RepairLayout R; RepairParams rp;
    if (const int st = stream_repair_resolve(m, s, max_gap, "uu3d_stream_commit_repair", c, R, rp)) return st;
    if (!state || !features || !active || !stage_frame || !stage_valid || !far_frames || !valid_state || !rows || !stride_mask || !fresh)
        return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_commit_repair: null buffer");
    if (((uintptr_t)state & 255) != 0 || ((uintptr_t)features & 15) != 0)
        return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_commit_repair: state must be 256-byte, features 16-byte aligned");
    c.base = (char*)state;
    const StreamParams p = stream_params(m, s, c.L);
    hipLaunchKernelGGL(stream_commit_repair_kernel, dim3(s->slots), dim3(256), 0, (hipStream_t)stream, p, R.K, max_gap, features, active,
                       (int32_t*)(c.base + c.L.off_frames), (float*)(c.base + c.L.off_table), stage_frame, stage_valid, far_frames, rows, stride_mask,
                       fresh, (uint8_t*)valid_state);
    return launched(m, "uu3d_stream_commit_repair");
}

int uu3d_stream_repair_reset(uu3d_model* m, const uu3d_stream_config* s, int32_t max_gap, void* repair_state, const uint8_t* slot_mask, void* stream) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c; RepairLayout R; RepairParams p;
    if (const int st = stream_repair_resolve(m, s, max_gap, "uu3d_stream_repair_reset", c, R, p)) return st;
    if (!repair_state || ((uintptr_t)repair_state & 255) != 0) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_repair_reset: repair_state must be a 256-byte aligned block");
    char* rb = (char*)repair_state;
    hipLaunchKernelGGL(stream_repair_reset_kernel, blocks_of((long)s->slots * p.J), dim3(256), 0, (hipStream_t)stream, slot_mask, s->slots, p.J,
                       (int32_t*)(rb + R.off_last), (uint32_t*)(rb + R.off_held));
    return launched(m, "uu3d_stream_repair_reset");
}

// ---- a session with a frame rate (uu3d_stream_rate.h): the state behind the plain session's and the launches around its sub-ticks ----
int uu3d_stream_rate_state_layout(const uu3d_model* mc, const uu3d_stream_config* s, const uu3d_stream_rate* r, uu3d_stream_rate_layout* out) {
    auto* m = const_cast<uu3d_model*>(mc);
    if (!m || !out) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c;
    if (const int st = stream_resolve(m, s, r, nullptr, nullptr, kStreamRate, "uu3d_stream_rate_state_layout", c)) return st;
    const RateLayout& R = c.R;
    out->source_frames_offset = (int64_t)R.off_source_frames; out->pushed_offset = (int64_t)R.off_pushed;
    out->source_valid_offset = (int64_t)R.off_source_valid; out->source_offset = (int64_t)R.off_source; out->keys_offset = (int64_t)R.off_keys;
    out->key_stride = R.key_stride; out->out_held_offset = (int64_t)R.off_out_held; out->bytes = (int64_t)R.bytes;
    return UU3D_OK;
}

int uu3d_stream_source_push(uu3d_model* m, const uu3d_stream_config* s, const uu3d_stream_rate* r, void* state, const float* kp,
                            const uint8_t* active, const uint8_t* valid_in, int32_t track_valid, void* stream) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c;
    if (const int st = stream_resolve(m, s, r, nullptr, state, kStreamRate | kStreamState, "uu3d_stream_source_push", c)) return st;
    if (!kp || !active || ((uintptr_t)kp & 7) != 0) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_source_push: kp (8-byte aligned) and active must be given");
    if (track_valid) if (const int st = stream_valid_check(m, "uu3d_stream_source_push")) return st;
    hipLaunchKernelGGL(stream_source_push_kernel, dim3(s->slots), dim3(64), 0, (hipStream_t)stream, kp, active, valid_in, track_valid ? 1 : 0,
                       m->cfg.num_keypoints, (int32_t*)(c.base + c.R.off_source_frames), (uint8_t*)(c.base + c.R.off_pushed),
                       (uint8_t*)(c.base + c.R.off_source_valid), (float*)(c.base + c.R.off_source));
    return launched(m, "uu3d_stream_source_push");
}

int uu3d_stream_resample_stage(uu3d_model* m, const uu3d_stream_config* s, const uu3d_stream_rate* r, const void* state, const double* resolution,
                               const int32_t* flip_order, uint8_t* sub_active, uint8_t* valid_out, float* frames_out, void* stream) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c;
    if (const int st = stream_resolve(m, s, r, nullptr, state, kStreamRate | kStreamState, "uu3d_stream_resample_stage", c)) return st;
    if (!sub_active || !frames_out || (s->flip && !flip_order)) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_resample_stage: null buffer");
    if (((uintptr_t)frames_out & 15) != 0) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_resample_stage: frames_out must be 16-byte aligned");
    if (valid_out) if (const int st = stream_valid_check(m, "uu3d_stream_resample_stage")) return st;
    const char* base = c.base;
    hipLaunchKernelGGL(stream_resample_stage_kernel, blocks_of(((long)c.L.halves * s->slots * m->cfg.num_keypoints + 1) / 2), dim3(256), 0,
                       (hipStream_t)stream, c.rate, (const int32_t*)(base + c.R.off_source_frames), (const int32_t*)(base + c.L.off_frames),
                       (const uint8_t*)(base + c.R.off_source_valid), (const float*)(base + c.R.off_source), resolution, flip_order, sub_active,
                       valid_out, frames_out);
    return launched(m, "uu3d_stream_resample_stage");
}

int uu3d_stream_file_keyframe(uu3d_model* m, const uu3d_stream_config* s, const uu3d_stream_rate* r, void* state, const uint8_t* fresh, void* stream) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c;
    if (const int st = stream_resolve(m, s, r, nullptr, state, kStreamRate | kStreamState, "uu3d_stream_file_keyframe", c)) return st;
    if (!fresh) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_file_keyframe: null fresh");
    hipLaunchKernelGGL(stream_file_keyframe_kernel, blocks_of((long)s->slots * (c.R.key_stride / 4)), dim3(256), 0, (hipStream_t)stream,
                       c.rate, (const int32_t*)(c.base + c.L.off_frames), fresh, (const float*)(c.base + c.L.off_held),
                       (float*)(c.base + c.R.off_keys));
    return launched(m, "uu3d_stream_file_keyframe");
}

int uu3d_stream_timed_emit(uu3d_model* m, const uu3d_stream_config* s, const uu3d_stream_rate* r, void* state, float* out, uint8_t* fresh_out,
                           void* stream) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c;
    if (const int st = stream_resolve(m, s, r, nullptr, state, kStreamRate | kStreamState, "uu3d_stream_timed_emit", c)) return st;
    if (!out || !fresh_out || ((uintptr_t)out & 15) != 0) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_timed_emit: out (16-byte aligned) and fresh_out must be given");
    hipLaunchKernelGGL(stream_timed_emit_kernel, blocks_of(((long)s->slots * c.L.per_pose + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                       c.rate, (const int32_t*)(c.base + c.R.off_source_frames), (const uint8_t*)(c.base + c.R.off_pushed),
                       (const float*)(c.base + c.R.off_keys), (float*)(c.base + c.R.off_out_held), out, fresh_out);
    return launched(m, "uu3d_stream_timed_emit");
}

int uu3d_stream_timed_emit_cubic(uu3d_model* m, const uu3d_stream_config* s, const uu3d_stream_rate* r, void* state, float* out, uint8_t* fresh_out,
                                 void* stream) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c;
    if (const int st = stream_resolve(m, s, r, nullptr, state, kStreamRate | kStreamState, "uu3d_stream_timed_emit_cubic", c)) return st;
    if (!out || !fresh_out || ((uintptr_t)out & 15) != 0) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_timed_emit_cubic: out (16-byte aligned) and fresh_out must be given");
    hipLaunchKernelGGL(stream_timed_emit_cubic_kernel, blocks_of(((long)s->slots * c.L.per_pose + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                       c.rate, (const int32_t*)(c.base + c.R.off_source_frames), (const uint8_t*)(c.base + c.R.off_pushed),
                       (const float*)(c.base + c.R.off_keys), (float*)(c.base + c.R.off_out_held), out, fresh_out);
    return launched(m, "uu3d_stream_timed_emit_cubic");
}

namespace {
// uu3d_stream_rate_reset and uu3d_stream_out_reset (with_out), behind their checks: one launch over the chosen slots
int stream_rate_reset(uu3d_model* m, const uu3d_stream_config* s, const StreamCall& c, const bool with_out, const uint8_t* slot_mask, void* stream,
                      const char* who) {
    hipLaunchKernelGGL(stream_rate_reset_kernel, blocks_of((long)s->slots * c.L.per_pose), dim3(256), 0, (hipStream_t)stream, slot_mask, s->slots,
                       c.L.per_pose, (int32_t*)(c.base + c.L.off_frames), (float*)(c.base + c.L.off_held), (int32_t*)(c.base + c.R.off_source_frames),
                       (uint8_t*)(c.base + c.R.off_pushed), (float*)(c.base + c.R.off_out_held),
                       with_out ? (int32_t*)(c.base + out_frames_offset(c.R)) : nullptr);
    return launched(m, who);
}
}  // namespace

int uu3d_stream_rate_reset(uu3d_model* m, const uu3d_stream_config* s, const uu3d_stream_rate* r, void* state, const uint8_t* slot_mask, void* stream) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c;
    if (const int st = stream_resolve(m, s, r, nullptr, state, kStreamRate | kStreamState, "uu3d_stream_rate_reset", c)) return st;
    return stream_rate_reset(m, s, c, false, slot_mask, stream, "uu3d_stream_rate_reset");
}

// ---- a session with an output rate of its own (StreamSession(fps=F, out_fps=G)): every due pose per push ----
int uu3d_stream_out_state_layout(const uu3d_model* mc, const uu3d_stream_config* s, const uu3d_stream_rate* r, const uu3d_stream_out* o,
                                 uu3d_stream_out_layout* out) {
    auto* m = const_cast<uu3d_model*>(mc);
    if (!m || !out) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c;
    if (const int st = stream_resolve(m, s, r, o, nullptr, kStreamRate | kStreamOut, "uu3d_stream_out_state_layout", c)) return st;
    out->out_frames_offset = (int64_t)out_frames_offset(c.R); out->bytes = (int64_t)out_layout_bytes(c.R, s->slots);
    return UU3D_OK;
}

int uu3d_stream_timed_emit_multi(uu3d_model* m, const uu3d_stream_config* s, const uu3d_stream_rate* r, const uu3d_stream_out* o, void* state,
                                 float* poses, int32_t* count, void* stream) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c;
    if (const int st = stream_resolve(m, s, r, o, state, kStreamRate | kStreamState | kStreamOut, "uu3d_stream_timed_emit_multi", c)) return st;
    if (!poses || !count || ((uintptr_t)poses & 15) != 0) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_timed_emit_multi: poses (16-byte aligned) and count must be given");
    hipLaunchKernelGGL(stream_timed_emit_multi_kernel, dim3(s->slots), dim3(256), 0, (hipStream_t)stream, c.rate, c.out,
                       (const int32_t*)(c.base + c.R.off_source_frames), (const uint8_t*)(c.base + c.R.off_pushed), (const float*)(c.base + c.R.off_keys),
                       (int32_t*)(c.base + out_frames_offset(c.R)), poses, count);
    return launched(m, "uu3d_stream_timed_emit_multi");
}

int uu3d_stream_timed_emit_multi_cubic(uu3d_model* m, const uu3d_stream_config* s, const uu3d_stream_rate* r, const uu3d_stream_out* o, void* state,
                                       float* poses, int32_t* count, void* stream) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c;
    if (const int st = stream_resolve(m, s, r, o, state, kStreamRate | kStreamState | kStreamOut, "uu3d_stream_timed_emit_multi_cubic", c)) return st;
    if (!poses || !count || ((uintptr_t)poses & 15) != 0) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_timed_emit_multi_cubic: poses (16-byte aligned) and count must be given");
    hipLaunchKernelGGL(stream_timed_emit_multi_cubic_kernel, dim3(s->slots), dim3(256), 0, (hipStream_t)stream, c.rate, c.out,
                       (const int32_t*)(c.base + c.R.off_source_frames), (const uint8_t*)(c.base + c.R.off_pushed), (const float*)(c.base + c.R.off_keys),
                       (int32_t*)(c.base + out_frames_offset(c.R)), poses, count);
    return launched(m, "uu3d_stream_timed_emit_multi_cubic");
}

int uu3d_stream_out_reset(uu3d_model* m, const uu3d_stream_config* s, const uu3d_stream_rate* r, const uu3d_stream_out* o, void* state,
                          const uint8_t* slot_mask, void* stream) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c;
    if (const int st = stream_resolve(m, s, r, o, state, kStreamRate | kStreamState | kStreamOut, "uu3d_stream_out_reset", c)) return st;
    return stream_rate_reset(m, s, c, true, slot_mask, stream, "uu3d_stream_out_reset");
}

// ---- LIVE ABSOLUTE ROOT (uu3d_stream_root.h): the ring of raw frames and the held root per slot, one launch per push, the reset ----
namespace {
// slots, joints and lookahead of a root call: UU3D_OK, or what is wrong (J beyond 64: UU3D_ERR_UNSUPPORTED)
int stream_root_resolve(const int32_t slots, const int32_t J, const int32_t lookahead, const void* state, RootRingLayout& L) {
    if (J > kRootMaxJoints) return UU3D_ERR_UNSUPPORTED;
    if (slots < 1 || slots > (1 << 20) || J < 1 || lookahead < 0 || lookahead > (1 << 24)) return UU3D_ERR_INVALID_ARGUMENT;
    if (!state || ((uintptr_t)state & 255) != 0) return UU3D_ERR_INVALID_ARGUMENT;
    L = root_ring_layout(slots, J, lookahead);
    return UU3D_OK;
}
}  // namespace

size_t uu3d_stream_root_bytes(int32_t slots, int32_t J, int32_t lookahead) {
    if (slots < 1 || slots > (1 << 20) || J < 1 || J > kRootMaxJoints || lookahead < 0 || lookahead > (1 << 24)) return 0;
    return root_ring_layout(slots, J, lookahead).bytes;
}

int uu3d_stream_root(int32_t slots, int32_t J, int32_t lookahead, void* root_state, const int32_t* frames, const uint8_t* active, const uint8_t* fresh,
                     const float* poses, const float* kp2d, const uint8_t* flags, int32_t flags_per_joint, const double* cameras, int32_t min_joints,
                     float* roots, uint8_t* root_state_out, void* stream) {
    RootRingLayout L;
    if (const int st = stream_root_resolve(slots, J, lookahead, root_state, L)) return st;
    if (!frames || !active || !fresh || !poses || !kp2d || !cameras || !roots || !root_state_out || min_joints < 2) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)frames & 3) != 0 || ((uintptr_t)poses & 3) != 0 || ((uintptr_t)kp2d & 7) != 0 || ((uintptr_t)cameras & 7) != 0 || ((uintptr_t)roots & 3) != 0)
        return UU3D_ERR_INVALID_ARGUMENT;
    char* b = (char*)root_state;
    hipLaunchKernelGGL(stream_root_kernel, dim3((unsigned)slots), dim3(64), 0, (hipStream_t)stream, J, L.W, frames, active, fresh, poses, kp2d, flags,
                       flags_per_joint != 0 ? 1 : 0, cameras, min_joints, (double*)(b + L.off_held), (float*)(b + L.off_kp), (uint8_t*)(b + L.off_used),
                       (uint8_t*)(b + L.off_last), roots, root_state_out);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_stream_root_reset(int32_t slots, int32_t J, int32_t lookahead, void* root_state, const uint8_t* slot_mask, void* stream) {
    RootRingLayout L;
    if (const int st = stream_root_resolve(slots, J, lookahead, root_state, L)) return st;
    char* b = (char*)root_state;
    hipLaunchKernelGGL(stream_root_reset_kernel, dim3((unsigned)slots), dim3(256), 0, (hipStream_t)stream, slot_mask, J, L.W, (double*)(b + L.off_held),
                       (float*)(b + L.off_kp), (uint8_t*)(b + L.off_used), (uint8_t*)(b + L.off_last));
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}
