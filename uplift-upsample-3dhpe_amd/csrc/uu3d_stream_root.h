// uu3d_stream_root.h -- LIVE ABSOLUTE ROOT (include/uu3d.h; stream.StreamSession(camera=...), stream.LiveRootHost): where the pose a live
// session returns must stand in the camera's space.  With a lookahead the pose of a push belongs to an earlier frame, so the session keeps
// the raw 2D of its last lookahead + 1 frames per slot and solves the pose against the frame it belongs to; a frame that cannot be solved
// takes the slot's last solved root (the rule is causal: no later pose exists to interpolate towards, unlike root_trajectory_kernel).
//     stream_root_kernel        per slot, one wave: lane j files joint j of the pushed frame, then lane 0 runs solve_root (uu3d_root.h) for
//                               the frame of the emitted pose and writes the root, its state and the held root
//     stream_root_reset_kernel  chosen slots: ring, held root and state back to zero
// Every output and state element has one writer, no atomics, the caller's buffers are only read: bitwise repeatable.
#pragma once
#include "uu3d_root.h"

namespace uu3d {

// The state block of a session's roots, per slot: the held root (3 f64, zeros until a frame is solved), a ring of W = lookahead + 1 raw
// frames (frame f at place f % W: J (x, y) pairs, as pushed, in the model's joint layout) with one USED byte per joint, and the state the
// slot returned last (0: no solved root yet, 1, 2) -- non-zero says that a solved root exists.
struct RootRingLayout {
    int W;
    size_t off_held, off_kp, off_used, off_last, bytes;
};
inline size_t root_ring_align(size_t v) { return (v + 255) / 256 * 256; }
inline RootRingLayout root_ring_layout(const int slots, const int J, const int lookahead)
{
    RootRingLayout L{};
    L.W = lookahead + 1;
    const size_t entries = (size_t)slots * (size_t)L.W * (size_t)J;
    L.off_held = 0;
    L.off_kp = root_ring_align((size_t)slots * 3 * sizeof(double));
    L.off_used = L.off_kp + root_ring_align(entries * 2 * sizeof(float));
    L.off_last = L.off_used + root_ring_align(entries);
    L.bytes = L.off_last + root_ring_align((size_t)slots);
    return L;
}

// The root of one slot at one tick, the work of ONE thread; shared by stream_root_kernel and stream_root_drain_kernel
// (uu3d_stream_drain.h).  solve: the slot's pose is fresh (and the slot takes part in the tick); have_frame: the frame the pose belongs to
// exists and may be read -- frame_kp (J, 2) as pushed, frame_used (J) u8 or nullptr.  Solved: held = the root, state 1.  Not solved (or no
// frame): state 2 when a held root exists, else 0.  !solve: what the slot returned last.  roots = the held root rounded once.
__device__ __forceinline__ void stream_root_settle(const int slot, const int J, const bool solve, const bool have_frame, const float* pose,
                                                   const float* frame_kp, const uint8_t* frame_used, const double* cam, const int min_joints,
                                                   double* __restrict__ held, uint8_t* __restrict__ last, float* __restrict__ roots,
                                                   uint8_t* __restrict__ root_state)
{
    uint8_t s = last[slot];
    double T[3] = {held[slot * 3], held[slot * 3 + 1], held[slot * 3 + 2]};
    if (solve) {
        double R[3] = {0.0, 0.0, 0.0};
        const bool ok = have_frame && solve_root(pose, frame_kp, frame_used, J, cam, min_joints, R);
        if (ok) {
            T[0] = R[0]; T[1] = R[1]; T[2] = R[2];
            held[slot * 3] = R[0]; held[slot * 3 + 1] = R[1]; held[slot * 3 + 2] = R[2];
            s = 1;
        } else s = s != 0 ? 2 : 0;
        last[slot] = s;
    }
    roots[slot * 3] = (float)T[0];
    roots[slot * 3 + 1] = (float)T[1];
    roots[slot * 3 + 2] = (float)T[2];
    root_state[slot] = s;
}

// One wave per slot.  frames (T) i32: the slot's frame counter AFTER this push (the pushed frame is t = frames - 1); active, fresh (T) u8;
// poses (T, J, 3) f32: the poses the push returns; kp (T, J, 2) f32: the pushed frames, raw; flags: nullptr, (T) u8 (per_joint == 0: a
// frame's flag stands for all of its joints) or (T, J) u8; cameras (T, 4) f64.
//   filing   an active slot: joint j of frame t into ring place t % W -- the pair as given, USED = flag and both coordinates finite.
//   solving  an active slot whose pose is fresh: frame c = t - (W - 1) against the pose.  c == t only when W == 1, and then lane 0 reads the
//            frame from kp and flags, not from the ring the other lanes are writing: no ordering between the lanes is needed.  Any other c
//            was filed by an earlier launch.  Solved: held = the root, state 1.  Not solved (or c < 0): state 2 when a held root exists, else 0.
//   any other slot returns what it returned last.  roots (T, 3) f32 = the held root rounded once; root_state (T) u8.
static __global__ void __launch_bounds__(64)
stream_root_kernel(const int J, const int W, const int32_t* __restrict__ frames, const uint8_t* __restrict__ active,
                   const uint8_t* __restrict__ fresh, const float* __restrict__ poses, const float* __restrict__ kp,
                   const uint8_t* __restrict__ flags, const int per_joint, const double* __restrict__ cameras, const int min_joints,
                   double* __restrict__ held, float* ring_kp, uint8_t* ring_used, uint8_t* __restrict__ last, float* __restrict__ roots,
                   uint8_t* __restrict__ root_state)
{
    const int slot = blockIdx.x, lane = threadIdx.x;
    const int count = frames[slot];
    const bool act = active[slot] != 0 && count >= 1;
    const int t = count - 1;
    const float* frame = kp + (long)slot * J * 2;
    const uint8_t* frame_flags = (flags != nullptr && per_joint != 0) ? flags + (long)slot * J : nullptr;
    const bool frame_flag = flags == nullptr || per_joint != 0 || flags[slot] != 0;
    if (act && lane < J) {
        const float2 uv = *reinterpret_cast<const float2*>(frame + 2 * lane);
        const bool flag = frame_flag && (frame_flags == nullptr || frame_flags[lane] != 0);
        const long e = ((long)slot * W + t % W) * J + lane;
        *reinterpret_cast<float2*>(ring_kp + 2 * e) = uv;
        ring_used[e] = (flag && finite_pair(uv)) ? 1 : 0;
    }
    if (lane != 0) return;

    const int c = t - (W - 1);
    const long e = ((long)slot * W + (c >= 0 ? c % W : 0)) * J;
    stream_root_settle(slot, J, act && fresh[slot] != 0, c >= 0 && (W != 1 || frame_flag), poses + (long)slot * J * 3,
                       W == 1 ? frame : ring_kp + 2 * e, W == 1 ? frame_flags : ring_used + e, cameras + 4 * (long)slot, min_joints, held, last,
                       roots, root_state);
}

// slot_mask (T) u8 or nullptr (every slot): the chosen slots have no filed frame, no held root and state 0.  One workgroup per slot.
static __global__ void __launch_bounds__(256)
stream_root_reset_kernel(const uint8_t* __restrict__ slot_mask, const int J, const int W, double* __restrict__ held, float* __restrict__ ring_kp,
                         uint8_t* __restrict__ ring_used, uint8_t* __restrict__ last)
{
    const int slot = blockIdx.x, tid = threadIdx.x;
    if (slot_mask != nullptr && slot_mask[slot] == 0) return;            // (uniform in the workgroup)
    const long per = (long)W * J, base = (long)slot * per;
    for (long i = tid; i < per; i += 256) {
        *reinterpret_cast<float2*>(ring_kp + 2 * (base + i)) = make_float2(0.f, 0.f);
        ring_used[base + i] = 0;
    }
    if (tid < 3) held[slot * 3 + tid] = 0.0;
    if (tid == 3) last[slot] = 0;
}

}  // namespace uu3d
