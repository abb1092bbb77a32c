// uu3d_associate.h -- PER-FRAME DETECTIONS (include/uu3d.h; predict.associate_detections / predict_detections,
// stream.StreamSession(detections=D)): the people a detector lists per frame, in any order -> tracks and slots, on the device.  ONE rule
// (predict.associate_host is the same rule in numpy, bit for bit): a normalised squared distance to each slot's reference pose, a greedy
// match with fixed tie-breaks, a slot lifecycle (born, aged, dead).  No motion model, no Hungarian step.
//   associate_frame          steps 1 to 6 of the rule for ONE frame, by one workgroup of 256 lanes (the device function both kernels call)
//   associate_step_kernel    one workgroup, one frame: the first launch of a live tick; it also scatters the detections into the session's
//                            frame, flags, active and born buffers
//   associate_video_kernel   one workgroup per video, its frames in order
// The small state of a frame (alive, age, track id, the seen joints of a slot as one 64-bit mask, the counters) lives in LDS while a kernel
// runs; the reference poses stay in the caller's state block.  S, D, K <= 64: the cost matrix is S x D 64-bit keys in LDS (32 KB), a
// detection's observed joints and a slot's seen joints are one 64-bit mask each.  Every output element has one writer, no atomics, the
// caller's detections are only read: bitwise repeatable.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "uu3d_tracks.h"

namespace uu3d {

static constexpr int kAssocMax = 64;                                    // the largest S, D and K
static constexpr int kAssocLanes = 256;
static constexpr uint64_t kAssocNoPair = ~0ull;                         // the key of a pair that is not allowed

struct AssocParams { int S, D, K, max_age, min_common; double max_dist2; };

// The state block: header (next_id, dropped) | track_id (S) i32 | age (S) i32 | seen (S) u64 | alive (S) u8 | ref (S, K, 2) f32
struct AssocLayout { size_t off_track, off_age, off_seen, off_alive, off_ref, bytes; };
__host__ __device__ inline AssocLayout assoc_layout(const int S, const int K)
{
    AssocLayout L;
    L.off_track = 16;
    L.off_age = L.off_track + (size_t)S * 4;
    L.off_seen = (L.off_age + (size_t)S * 4 + 7) / 8 * 8;
    L.off_alive = L.off_seen + (size_t)S * 8;
    L.off_ref = (L.off_alive + (size_t)S + 7) / 8 * 8;
    L.bytes = (L.off_ref + (size_t)S * K * 8 + 255) / 256 * 256;
    return L;
}

// What a workgroup keeps in LDS.  key[s * D + d]: the cost of the pair as an order-preserving 64-bit integer (a non-negative double's own
// bits), kAssocNoPair where the pair is not allowed.
struct AssocShared {
    uint64_t key[kAssocMax * kAssocMax];
    uint64_t seen[kAssocMax], obs[kAssocMax];                           // joints seen since a slot's birth; joints observed in a detection
    double scale2[kAssocMax];
    int32_t track[kAssocMax], age[kAssocMax], slot_det[kAssocMax], det_slot[kAssocMax];
    uint8_t alive[kAssocMax], born[kAssocMax], cand[kAssocMax], full[kAssocMax];   // full: every joint flag of the detection is set
    uint64_t red_key[4];
    int32_t red_idx[4];
    int32_t next_id, dropped;
};

// sum over the common joints, ascending, of dx * dx + dy * dy in float64: every product and every sum rounded, no fused multiply-add
__device__ __forceinline__ double assoc_add_joint(const double acc, const float2 det, const float2 ref)
{
#pragma clang fp contract(off)
    const double dx = (double)det.x - (double)ref.x;
    const double dy = (double)det.y - (double)ref.y;
    const double xx = dx * dx;
    const double yy = dy * dy;
    const double term = xx + yy;
    return acc + term;
}
// w * w + h * h of a slot's bounding box, and the cost's one division
__device__ __forceinline__ double assoc_scale2(const float x0, const float x1, const float y0, const float y1)
{
#pragma clang fp contract(off)
    const double w = (double)x1 - (double)x0;
    const double h = (double)y1 - (double)y0;
    const double ww = w * w;
    const double hh = h * h;
    return ww + hh;
}
__device__ __forceinline__ double assoc_cost(const double d2, const int n, const double scale2)
{
#pragma clang fp contract(off)
    const double den = (double)n * scale2;
    return d2 / den;
}

__device__ __forceinline__ uint64_t assoc_shfl_xor(const uint64_t v, const int m)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
    return ((uint64_t)hi << 32) | lo;
}

// One frame.  dets (D, K, 2) f32; count: detections given (clamped into [0, D]); flags: nullptr, (D,) u8 (flag_joints == 0) or (D, K) u8.
// ref: the state block's reference poses (S, K, 2).  sh holds the state on entry and on return; after the call sh.slot_det[s] is the
// detection that is slot s's frame of this tick (-1: none), sh.det_slot[d] the assignment, sh.born the births.  Ends with a barrier.
__device__ inline void associate_frame(AssocShared& sh, const AssocParams& p, const float* __restrict__ dets, int count, const uint8_t* __restrict__ flags,
                                       const int flag_joints, float* __restrict__ ref)
{
    const int lane = threadIdx.x, S = p.S, D = p.D, K = p.K;
    count = count < 0 ? 0 : (count > D ? D : count);
    // a. per detection: the observed joints and whether it is a candidate; per slot: the scale of its reference pose
    if (lane < D) {
        const int d = lane;
        uint64_t obs = 0;
        bool full = true;
        const bool frame_flag = flags == nullptr || flag_joints != 0 || flags[d] != 0;
        for (int j = 0; j < K; ++j) {
            const bool flag = flags == nullptr || flag_joints == 0 || flags[d * K + j] != 0;
            full = full && flag;
            if (flag && finite_pair(*reinterpret_cast<const float2*>(dets + ((long)d * K + j) * 2))) obs |= 1ull << j;
        }
        sh.obs[d] = obs;
        sh.full[d] = full ? 1 : 0;
        sh.cand[d] = (d < count && frame_flag && __popcll(obs) >= p.min_common) ? 1 : 0;
        sh.det_slot[d] = -1;
    }
    if (lane >= 64 && lane < 64 + S) {
        const int s = lane - 64;
        double scale2 = 0.0;
        const uint64_t seen = sh.seen[s];
        if (sh.alive[s] != 0 && seen != 0) {
            float x0 = 0.f, x1 = 0.f, y0 = 0.f, y1 = 0.f;
            bool first = true;
            for (int j = 0; j < K; ++j) {
                if (!((seen >> j) & 1)) continue;
                const float2 r = *reinterpret_cast<const float2*>(ref + ((long)s * K + j) * 2);
                if (first) { x0 = x1 = r.x; y0 = y1 = r.y; first = false; }
                else { x0 = r.x < x0 ? r.x : x0; x1 = r.x > x1 ? r.x : x1; y0 = r.y < y0 ? r.y : y0; y1 = r.y > y1 ? r.y : y1; }
            }
            scale2 = assoc_scale2(x0, x1, y0, y1);
        }
        sh.scale2[s] = scale2;
        sh.slot_det[s] = -1;
        sh.born[s] = 0;
    }
    __syncthreads();
    // b. the cost of every (alive slot, candidate) pair, the joint loop in ascending order
    for (int q = lane; q < S * D; q += kAssocLanes) {
        const int s = q / D, d = q - s * D;
        uint64_t key = kAssocNoPair;
        if (sh.alive[s] != 0 && sh.cand[d] != 0) {
            const uint64_t common = sh.seen[s] & sh.obs[d];
            const int n = __popcll(common);
            const double scale2 = sh.scale2[s];
            if (n >= p.min_common && n > 0 && scale2 != 0.0) {
                double d2 = 0.0;
                for (int j = 0; j < K; ++j) {
                    if (!((common >> j) & 1)) continue;
                    d2 = assoc_add_joint(d2, *reinterpret_cast<const float2*>(dets + ((long)d * K + j) * 2),
                                         *reinterpret_cast<const float2*>(ref + ((long)s * K + j) * 2));
                }
                const double cost = assoc_cost(d2, n, scale2);
                if (cost <= p.max_dist2) key = (uint64_t)__double_as_longlong(cost);
            }
        }
        sh.key[q] = key;
    }
    __syncthreads();
    // c. greedy: the allowed pair of smallest (cost, s, d) among unmatched slots and candidates, until none is left
    for (int round = 0; round < kAssocMax; ++round) {
        uint64_t best = kAssocNoPair;
        int best_idx = 0x7fffffff;
        for (int q = lane; q < S * D; q += kAssocLanes) {
            const int s = q / D, d = q - s * D;
            const uint64_t key = sh.key[q];
            const int idx = s * kAssocMax + d;
            if (key != kAssocNoPair && sh.slot_det[s] < 0 && sh.det_slot[d] < 0 && (key < best || (key == best && idx < best_idx))) { best = key; best_idx = idx; }
        }
        for (int m = 32; m >= 1; m >>= 1) {
            const uint64_t other = assoc_shfl_xor(best, m);
            const int other_idx = __shfl_xor(best_idx, m);
            if (other < best || (other == best && other_idx < best_idx)) { best = other; best_idx = other_idx; }
        }
        if ((lane & 63) == 0) { sh.red_key[lane >> 6] = best; sh.red_idx[lane >> 6] = best_idx; }
        __syncthreads();
        best = sh.red_key[0]; best_idx = sh.red_idx[0];
        for (int w = 1; w < 4; ++w) {
            const uint64_t other = sh.red_key[w];
            const int other_idx = sh.red_idx[w];
            if (other < best || (other == best && other_idx < best_idx)) { best = other; best_idx = other_idx; }
        }
        __syncthreads();                                               // (everyone has read the four candidates before they are rewritten)
        if (best == kAssocNoPair) break;                               // (the same value in every lane)
        if (lane == 0) { sh.slot_det[best_idx / kAssocMax] = best_idx % kAssocMax; sh.det_slot[best_idx % kAssocMax] = best_idx / kAssocMax; }
        __syncthreads();
    }
    // d. matched slots are young again, unmatched ones age and die
    if (lane < S && sh.alive[lane] != 0) {
        const int s = lane;
        if (sh.slot_det[s] >= 0) sh.age[s] = 0;
        else {
            const int age = sh.age[s] + 1;
            sh.age[s] = age;
            if (age > p.max_age) { sh.alive[s] = 0; sh.track[s] = -1; sh.age[s] = 0; sh.seen[s] = 0; }
        }
    }
    __syncthreads();
    // e. births: the unmatched candidates in ascending d take the free slots in ascending s (wave 0: lane = detection and lane = slot)
    if (lane < 64) {
        const bool unmatched = lane < D && sh.cand[lane] != 0 && sh.det_slot[lane] < 0;
        const bool is_free = lane < S && sh.alive[lane] == 0;
        const uint64_t want = __ballot(unmatched), room = __ballot(is_free);
        const int n_want = __popcll(want), n_room = __popcll(room);
        if (unmatched) {
            const int rank = __popcll(want & ((1ull << lane) - 1ull));
            if (rank < n_room) {
                uint64_t m = room;
                for (int i = 0; i < rank; ++i) m &= m - 1;             // drop the `rank` lowest free slots
                const int s = __ffsll((unsigned long long)m) - 1;
                sh.det_slot[lane] = s;
                sh.slot_det[s] = lane;
                sh.born[s] = 1;
                sh.alive[s] = 1;
                sh.age[s] = 0;
                sh.seen[s] = 0;
                sh.track[s] = sh.next_id + rank;
            }
        }
        if (lane == 0) {
            const int made = n_want < n_room ? n_want : n_room;
            sh.next_id += made;
            sh.dropped += n_want - made;
        }
    }
    __syncthreads();
    // f. the reference pose of a slot with a detection takes the observed joints' bits
    for (int q = lane; q < S * K; q += kAssocLanes) {
        const int s = q / K, j = q - s * K;
        const int d = sh.slot_det[s];
        if (d >= 0 && ((sh.obs[d] >> j) & 1))
            *reinterpret_cast<float2*>(ref + (long)q * 2) = *reinterpret_cast<const float2*>(dets + ((long)d * K + j) * 2);
    }
    __syncthreads();                                                   // (the loop above reads no seen mask; the next lines write them)
    if (lane < S && sh.slot_det[lane] >= 0) sh.seen[lane] |= sh.obs[sh.slot_det[lane]];
    __syncthreads();
}

__device__ inline void assoc_load_state(AssocShared& sh, const AssocLayout& L, const int S, const char* state)
{
    const int lane = threadIdx.x;
    if (lane < S) {
        sh.track[lane] = reinterpret_cast<const int32_t*>(state + L.off_track)[lane];
        sh.age[lane] = reinterpret_cast<const int32_t*>(state + L.off_age)[lane];
        sh.seen[lane] = reinterpret_cast<const uint64_t*>(state + L.off_seen)[lane];
        sh.alive[lane] = reinterpret_cast<const uint8_t*>(state + L.off_alive)[lane];
    }
    if (lane == 0) { sh.next_id = reinterpret_cast<const int32_t*>(state)[0]; sh.dropped = reinterpret_cast<const int32_t*>(state)[1]; }
    __syncthreads();
}
__device__ inline void assoc_store_state(const AssocShared& sh, const AssocLayout& L, const int S, char* state)
{
    const int lane = threadIdx.x;
    if (lane < S) {
        reinterpret_cast<int32_t*>(state + L.off_track)[lane] = sh.track[lane];
        reinterpret_cast<int32_t*>(state + L.off_age)[lane] = sh.age[lane];
        reinterpret_cast<uint64_t*>(state + L.off_seen)[lane] = sh.seen[lane];
        reinterpret_cast<uint8_t*>(state + L.off_alive)[lane] = sh.alive[lane];
    }
    if (lane == 0) { reinterpret_cast<int32_t*>(state)[0] = sh.next_id; reinterpret_cast<int32_t*>(state)[1] = sh.dropped; }
}

// The live tick's first launch: one workgroup, one frame.  count (1) i32 on the device.  Besides the rule's outputs it writes what the rest
// of the tick reads: kp_out (S, K, 2) = the slot's detection (zeros without one); flags_out (S, K) (flags_out_joints != 0: a joint's byte is
// 1 iff it is observed) or (S,) (1 iff the slot has a detection and every joint flag of it is set); active_out (S) = alive; born_out (S).
static __global__ void __launch_bounds__(kAssocLanes)
associate_step_kernel(const AssocParams p, char* __restrict__ state, const float* __restrict__ dets, const int32_t* __restrict__ count,
                      const uint8_t* __restrict__ flags, const int flag_joints, float* __restrict__ kp_out, uint8_t* __restrict__ flags_out,
                      const int flags_out_joints, uint8_t* __restrict__ active_out, uint8_t* __restrict__ born_out, int32_t* __restrict__ assignment,
                      int32_t* __restrict__ track_ids, int32_t* __restrict__ dropped)
{
    __shared__ AssocShared sh;
    const AssocLayout L = assoc_layout(p.S, p.K);
    const int lane = threadIdx.x, S = p.S, D = p.D, K = p.K;
    assoc_load_state(sh, L, S, state);
    associate_frame(sh, p, dets, count[0], flags, flag_joints, reinterpret_cast<float*>(state + L.off_ref));
    assoc_store_state(sh, L, S, state);
    if (lane < D) assignment[lane] = sh.det_slot[lane];
    if (lane < S) {
        const int d = sh.slot_det[lane];
        track_ids[lane] = sh.track[lane];
        active_out[lane] = sh.alive[lane];
        born_out[lane] = sh.born[lane];
        if (flags_out_joints == 0) flags_out[lane] = (d >= 0 && sh.full[d] != 0) ? 1 : 0;
    }
    if (lane == 0) dropped[0] = sh.dropped;
    for (int q = lane; q < S * K; q += kAssocLanes) {
        const int s = q / K, j = q - s * K;
        const int d = sh.slot_det[s];
        float2 v = make_float2(0.f, 0.f);
        if (d >= 0) v = *reinterpret_cast<const float2*>(dets + ((long)d * K + j) * 2);
        *reinterpret_cast<float2*>(kp_out + (long)q * 2) = v;
        if (flags_out_joints != 0) flags_out[q] = (d >= 0 && ((sh.obs[d] >> j) & 1)) ? 1 : 0;
    }
}

// Whole videos: workgroup v takes frames [video_start[v], video_start[v + 1]) in order, from a fresh state, and leaves the final state in
// its own block of `state` (stride assoc_layout(S, K).bytes) and (next_id, dropped) in counters (V, 2).  Per frame: assignment (F, D),
// track_of (F, D) = the track id of each detection or -1, and, where given, track_ids (F, S), born (F, S), alive (F, S).
static __global__ void __launch_bounds__(kAssocLanes)
associate_video_kernel(const AssocParams p, const float* __restrict__ dets, const int32_t* __restrict__ counts, const uint8_t* __restrict__ flags,
                       const int flag_joints, const int64_t* __restrict__ video_start, const long frames, char* __restrict__ state,
                       int32_t* __restrict__ assignment, int32_t* __restrict__ track_of, int32_t* __restrict__ track_ids, uint8_t* __restrict__ born,
                       uint8_t* __restrict__ alive, int32_t* __restrict__ counters)
{
    __shared__ AssocShared sh;
    const AssocLayout L = assoc_layout(p.S, p.K);
    const int lane = threadIdx.x, S = p.S, D = p.D, K = p.K;
    char* my = state + (size_t)blockIdx.x * L.bytes;
    if (lane < S) { sh.track[lane] = -1; sh.age[lane] = 0; sh.seen[lane] = 0; sh.alive[lane] = 0; }
    if (lane == 0) { sh.next_id = 0; sh.dropped = 0; }
    __syncthreads();
    long f0 = video_start[blockIdx.x], f1 = video_start[blockIdx.x + 1];
    f0 = f0 < 0 ? 0 : f0;
    f1 = f1 > frames ? frames : f1;
    for (long f = f0; f < f1; ++f) {
        const uint8_t* fl = flags == nullptr ? nullptr : flags + (flag_joints != 0 ? f * D * K : f * D);
        associate_frame(sh, p, dets + f * D * K * 2, counts == nullptr ? D : counts[f], fl, flag_joints, reinterpret_cast<float*>(my + L.off_ref));
        if (lane < D) {
            const int s = sh.det_slot[lane];
            assignment[f * D + lane] = s;
            track_of[f * D + lane] = s >= 0 ? sh.track[s] : -1;
        }
        if (lane < S) {
            if (track_ids != nullptr) track_ids[f * S + lane] = sh.track[lane];
            if (born != nullptr) born[f * S + lane] = sh.born[lane];
            if (alive != nullptr) alive[f * S + lane] = sh.alive[lane];
        }
        __syncthreads();                                               // (the next frame's first phase rewrites what was just read)
    }
    assoc_store_state(sh, L, S, my);
    if (lane == 0) { counters[2 * blockIdx.x] = sh.next_id; counters[2 * blockIdx.x + 1] = sh.dropped; }
}

// chosen slots (nullptr: every slot, and the counters) back to free
static __global__ void __launch_bounds__(64)
associate_reset_kernel(const int S, const int K, char* __restrict__ state, const uint8_t* __restrict__ slot_mask)
{
    const AssocLayout L = assoc_layout(S, K);
    const int lane = threadIdx.x;
    if (lane < S && (slot_mask == nullptr || slot_mask[lane] != 0)) {
        reinterpret_cast<int32_t*>(state + L.off_track)[lane] = -1;
        reinterpret_cast<int32_t*>(state + L.off_age)[lane] = 0;
        reinterpret_cast<uint64_t*>(state + L.off_seen)[lane] = 0;
        reinterpret_cast<uint8_t*>(state + L.off_alive)[lane] = 0;
    }
    if (lane == 0 && slot_mask == nullptr) { reinterpret_cast<int32_t*>(state)[0] = 0; reinterpret_cast<int32_t*>(state)[1] = 0; }
}

}  // namespace uu3d
