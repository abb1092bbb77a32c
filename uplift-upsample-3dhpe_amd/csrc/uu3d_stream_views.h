// uu3d_stream_views.h -- LIVE SEVERAL VIEWS (include/uu3d.h; stream.StreamSession(views=V), stream.LiveViewsHost): SEVERAL VIEWS for LIVE
// TRACKS.  The slots of a session are view-major -- slot v * N + i is person i in camera v --, uu3d_stream_root has filed every slot's
// raw frame in its ring and uu3d_camera_to_world has left every slot's pose in world axes; this file joins the V slots of a person to one
// pose and ONE world root per push.  A push is the clock: what the slots received at one push is one instant.
//     stream_views_kernel        per person, one wave: lane j fuses joint j over the views (uu3d_views.h's rule, one 12-byte store), the
//                                fused pose goes through LDS to lane 0, which runs solve_view_root_at against every seeing view's own ring
//                                frame and settles the root as stream_root_settle does
//     stream_views_reset_kernel  the persons ALL of whose slots are chosen: held root, state and tick counter back to zero
// The ring of uu3d_stream_root.h is only read, in a later launch than the one that filed it.  Every output and state element has one
// writer, no atomics: bitwise repeatable.  The views are walked through bit masks; nothing is indexed per lane by a run-time view number.
#pragma once
#include "uu3d_stream_root.h"
#include "uu3d_views.h"

namespace uu3d {

// The state block of a session's persons: the held world root (3 f64, zeros until a tick is solved), the state the person returned last
// (0: no solved root yet, 1, 2) and the person's tick counter.
struct ViewsStateLayout {
    size_t off_held, off_last, off_ticks, bytes;
};
inline ViewsStateLayout views_state_layout(const int persons)
{
    ViewsStateLayout L{};
    L.off_held = 0;
    L.off_last = root_ring_align((size_t)persons * 3 * sizeof(double));
    L.off_ticks = L.off_last + root_ring_align((size_t)persons);
    L.bytes = L.off_ticks + root_ring_align((size_t)persons * sizeof(int32_t));
    return L;
}

// Where joint 0 of the frame of view v's pose lies in the ring's (slots, W, J) planes: frame c = frames[slot] - 1 - (W - 1) at place c % W.
// Only asked for views whose c >= 0.
struct RingFrames {
    const int32_t* frames;
    int persons, person, W, J;
    __device__ __forceinline__ long operator()(const int v) const
    {
        const int slot = v * persons + person;
        const int c = frames[slot] - W;
        return ((long)slot * W + c % W) * J;
    }
};

// One wave per person.  frames / active / fresh (V N): the slots' counters AFTER this push, who took part in it, whose pose is new;
// view_poses (V N, J, 3) f32: the slots' poses in world axes; ring_kp / ring_used: uu3d_stream_root's ring; cams (V, 16) f64.
//   view v TAKES PART iff its slot is active (frames >= 1) and fresh; it SEES iff it takes part, its frame c >= 0 and at least min_joints
//   USED bytes are set there.  A person is fresh iff a view takes part: the pose is the float64 mean over the seeing views in ascending
//   order, rounded once -- nobody sees: over the views that take part, view_count 0 --, and the root is solved against it.  Solved: held =
//   the root, state 1; not solved: state 2 when a held root exists, else 0.  A person that is not fresh keeps its pose row and returns the
//   held root and its last state, view_count 0.  The tick counter grows by one iff any slot of the person is active.
static __global__ void __launch_bounds__(64)
stream_views_kernel(const int views, const int persons, const int J, const int W, const int32_t* __restrict__ frames,
                    const uint8_t* __restrict__ active, const uint8_t* __restrict__ fresh, const float* __restrict__ view_poses,
                    const float* __restrict__ ring_kp, const uint8_t* __restrict__ ring_used, const double* __restrict__ cams, const int min_joints,
                    double* __restrict__ held, uint8_t* __restrict__ last, int32_t* __restrict__ ticks, float* __restrict__ poses,
                    uint8_t* __restrict__ fresh_out, float* __restrict__ roots, uint8_t* __restrict__ root_state, uint8_t* __restrict__ view_count,
                    int32_t* __restrict__ person_frames, uint8_t* __restrict__ person_active)
{
#pragma clang fp contract(off)
    __shared__ float fused[kRootMaxJoints * 3];
    const int person = blockIdx.x, lane = threadIdx.x;
    unsigned part = 0, placed = 0;
    bool any_active = false;
    for (int v = 0; v < views; ++v) {                                    // (uniform in the wave)
        const int slot = v * persons + person;
        const int count = frames[slot];
        const bool act = active[slot] != 0;
        any_active = any_active || act;
        if (act && count >= 1 && fresh[slot] != 0) {
            part |= 1u << v;
            if (count >= W) placed |= 1u << v;                           // c = count - 1 - (W - 1) >= 0: the frame is in the ring
        }
    }
    const RingFrames at{frames, persons, person, W, J};
    const unsigned mask = seeing_views_at(ring_kp, ring_used, at, placed, views, J, min_joints);
    const int seen = __popc(mask);
    const unsigned take = seen > 0 ? mask : part;
    const int n = seen > 0 ? seen : __popc(part);
    if (part != 0 && lane < J) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int v = 0; v < views; ++v) {
            if (((take >> v) & 1u) == 0) continue;
            const WorldTrio t = *reinterpret_cast<const WorldTrio*>(view_poses + (((long)v * persons + person) * J + lane) * 3);
            s0 = s0 + (double)t.a;
            s1 = s1 + (double)t.b;
            s2 = s2 + (double)t.c;
        }
        const double nd = (double)n;
        WorldTrio r;
        r.a = (float)(s0 / nd);
        r.b = (float)(s1 / nd);
        r.c = (float)(s2 / nd);
        *reinterpret_cast<WorldTrio*>(poses + ((long)person * J + lane) * 3) = r;
        fused[3 * lane] = r.a;
        fused[3 * lane + 1] = r.b;
        fused[3 * lane + 2] = r.c;
    }
    __syncthreads();
    if (lane != 0) return;

    uint8_t s = last[person];
    double T[3] = {held[person * 3], held[person * 3 + 1], held[person * 3 + 2]};
    if (part != 0) {
        double R[3] = {0.0, 0.0, 0.0};
        if (solve_view_root_at(fused, ring_kp, ring_used, at, mask, views, J, cams, R)) {
            T[0] = R[0]; T[1] = R[1]; T[2] = R[2];
            held[person * 3] = R[0]; held[person * 3 + 1] = R[1]; held[person * 3 + 2] = R[2];
            s = 1;
        } else s = s != 0 ? 2 : 0;
        last[person] = s;
    }
    roots[person * 3] = (float)T[0];
    roots[person * 3 + 1] = (float)T[1];
    roots[person * 3 + 2] = (float)T[2];
    root_state[person] = s;
    fresh_out[person] = part != 0 ? 1 : 0;
    view_count[person] = (uint8_t)(part != 0 ? seen : 0);
    const int32_t now = ticks[person] + (any_active ? 1 : 0);
    ticks[person] = now;
    person_frames[person] = now;
    person_active[person] = any_active ? 1 : 0;
}

// slot_mask (V N) u8 or nullptr (every slot): a person ALL of whose V slots are chosen has no held root, state 0 and tick counter 0.  One
// lane per person.
static __global__ void __launch_bounds__(256)
stream_views_reset_kernel(const uint8_t* __restrict__ slot_mask, const int views, const int persons, double* __restrict__ held,
                          uint8_t* __restrict__ last, int32_t* __restrict__ ticks)
{
    const int person = blockIdx.x * 256 + threadIdx.x;
    if (person >= persons) return;
    if (slot_mask != nullptr)
        for (int v = 0; v < views; ++v)
            if (slot_mask[v * persons + person] == 0) return;
    held[person * 3] = 0.0;
    held[person * 3 + 1] = 0.0;
    held[person * 3 + 2] = 0.0;
    last[person] = 0;
    ticks[person] = 0;
}

}  // namespace uu3d
