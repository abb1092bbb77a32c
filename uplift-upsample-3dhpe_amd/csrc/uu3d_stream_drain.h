// uu3d_stream_drain.h -- LIVE TRACKS: END OF A TRACK (include/uu3d.h; stream.StreamSession.finish): a session with lookahead a answers a push
// with the pose of frame newest - a, so a track that ends still owes the poses of its last a frames.  A DRAIN TICK advances the window's
// centre by one frame towards the newest one WITHOUT filing a frame; everything it reads is still in the session's state (the keyframe
// ring covers centre - half span .. newest, the edge row is the last one filed, the root ring holds the raw frames newest - a .. newest).
//   stream_drain_commit_kernel  per slot: advance `drained`, write the window of centre frames - 1 - lookahead + drained (stream_write_window
//                               of uu3d_stream.h with a centre offset: frames behind the track's end are padded as the end of a video is)
//   stream_root_drain_kernel    stream_root_kernel's solve (stream_root_settle of uu3d_stream_root.h) for the frame of the drained pose, read
//                               from the ring; nothing is filed
//   stream_drain_file_kernel    the tick's buffers (slots, w) -> row drained - 1 of the result buffers (slots, lookahead, w)
//   stream_drain_reset_kernel   chosen slots: drain state back to zero
// The per-slot drain state is a small block of its own (DrainLayout), not part of StreamLayout: a session that never finishes a track
// allocates none of it.  No atomics, every output and state element has one writer, the row index comes from the device counter: the
// launches of a drain tick have the same arguments at every tick and replay from one captured graph.
#pragma once
#include "uu3d_stream.h"
#include "uu3d_stream_root.h"

namespace uu3d {

// Per slot: drained (i32) -- drain ticks taken since the slot's last reset, at most lookahead --, virtual_frames (i32) = frames + drained:
// the counter the frame of the drained pose is counted from (c = virtual_frames - 1 - lookahead), what the root solve and the filters
// take in place of the frame counter --, ticked (u8): the slot advanced at the last drain tick.
struct DrainLayout {
    size_t off_drained, off_virtual, off_ticked, bytes;
};
inline DrainLayout drain_layout(const int slots)
{
    DrainLayout L{};
    L.off_drained = 0;
    L.off_virtual = stream_align((size_t)slots * sizeof(int32_t));
    L.off_ticked = L.off_virtual + stream_align((size_t)slots * sizeof(int32_t));
    L.bytes = L.off_ticked + stream_align((size_t)slots);
    return L;
}

// One workgroup per slot.  chosen (T) u8: the slots whose tracks have ended.  A chosen slot with frames >= 1 and drained < lookahead
// advances `drained` and gets the window of centre frames - 1 - lookahead + drained; it files NOTHING -- no feature row, no validity byte,
// and `frames` is only read.  Any other slot gets the all-masked, not-fresh window of an inactive slot.  The slot's counters are read by
// every thread of ITS workgroup only, and written by one of them behind a barrier (stream_commit_kernel's discipline).  valid_state:
// nullptr, or the session's validity bytes (missed detections, repair_joints), only read.
static __global__ void __launch_bounds__(256)
stream_drain_commit_kernel(const StreamParams p, const uint8_t* __restrict__ chosen, const int32_t* __restrict__ frames,
                           int32_t* __restrict__ drained, int32_t* __restrict__ virtual_frames, uint8_t* __restrict__ ticked,
                           int32_t* __restrict__ rows, uint8_t* __restrict__ stride_mask, uint8_t* __restrict__ fresh, const uint8_t* valid_state)
{
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int len = frames[slot], before = drained[slot];
    const bool act = chosen[slot] != 0 && len >= 1 && before >= 0 && before < p.lookahead;
    __syncthreads();                                                     // every read of the counters is done
    const int k = before + (act ? 1 : 0);
    if (tid == 0) {
        if (act) drained[slot] = k;
        const long v = (long)len + (long)k;
        virtual_frames[slot] = v > INT32_MAX ? INT32_MAX : (int32_t)v;
        ticked[slot] = act ? 1 : 0;
    }
    stream_write_window(p, slot, tid, len, act, k, valid_state, rows, stride_mask, fresh);
}

// One thread per slot (the solve is lane 0's work in stream_root_kernel as well).  virtual_frames (T) i32 of the drain state; chosen, fresh
// (T) u8; poses (T, J, 3) f32: the poses of this drain tick.  A chosen slot whose pose is fresh: frame c = virtual_frames - 1 - (W - 1) --
// one of the last W frames filed, so it is read from the ring -- against the pose, by stream_root_kernel's rule (held root, states).  Any
// other slot returns what it returned last.  No lane files anything.
static __global__ void __launch_bounds__(64)
stream_root_drain_kernel(const int T, const int J, const int W, const int32_t* __restrict__ virtual_frames, const uint8_t* __restrict__ chosen,
                         const uint8_t* __restrict__ fresh, const float* __restrict__ poses, const double* __restrict__ cameras,
                         const int min_joints, double* __restrict__ held, const float* __restrict__ ring_kp,
                         const uint8_t* __restrict__ ring_used, uint8_t* __restrict__ last, float* __restrict__ roots,
                         uint8_t* __restrict__ root_state)
{
    const int slot = blockIdx.x * 64 + threadIdx.x;
    if (slot >= T) return;
    const int c = virtual_frames[slot] - 1 - (W - 1);
    const bool solve = chosen[slot] != 0 && fresh[slot] != 0;
    const long e = ((long)slot * W + (c >= 0 ? c % W : 0)) * J;
    stream_root_settle(slot, J, solve, c >= 0, poses + (long)slot * J * 3, ring_kp + 2 * e, ring_used + e, cameras + 4 * (long)slot, min_joints,
                       held, last, roots, root_state);
}

// What stream_drain_file_kernel scatters: up to kDrainFileBuffers float buffers (T, width) -> (T, A, width), and up to two byte buffers
// (T) -> (T, A).  Unused entries are nullptr / width 0.
static constexpr int kDrainFileBuffers = 4;
struct DrainFileParams {
    const float* src[kDrainFileBuffers];
    float* dst[kDrainFileBuffers];
    int width[kDrainFileBuffers];
    const uint8_t* byte_src[2];
    uint8_t* byte_dst[2];
};

// One workgroup per slot.  A slot that advanced at this drain tick (ticked) files the tick's rows into row drained - 1 of the result
// buffers; any other slot writes nothing.  A is the rows per slot (the lookahead).  Every element has one writer.
static __global__ void __launch_bounds__(256)
stream_drain_file_kernel(const DrainFileParams f, const int A, const int32_t* __restrict__ drained, const uint8_t* __restrict__ ticked)
{
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int row = drained[slot] - 1;
    if (ticked[slot] == 0 || row < 0 || row >= A) return;               // (uniform in the workgroup)
#pragma unroll
    for (int b = 0; b < kDrainFileBuffers; ++b) {
        const int w = f.width[b];
        if (f.src[b] == nullptr || w < 1) continue;
        const float* s = f.src[b] + (size_t)slot * w;
        float* d = f.dst[b] + ((size_t)slot * A + row) * w;
        for (int i = tid; i < w; i += 256) d[i] = s[i];
    }
    if (tid < 2 && f.byte_src[tid] != nullptr) f.byte_dst[tid][(size_t)slot * A + row] = f.byte_src[tid][slot];
}

// slot_mask (T) u8 or nullptr (every slot): the chosen slots have drained nothing.
static __global__ void __launch_bounds__(256)
stream_drain_reset_kernel(const uint8_t* __restrict__ slot_mask, const int T, int32_t* __restrict__ drained, int32_t* __restrict__ virtual_frames,
                          uint8_t* __restrict__ ticked)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    if (slot_mask != nullptr && slot_mask[t] == 0) return;
    drained[t] = 0;
    virtual_frames[t] = 0;
    ticked[t] = 0;
}

}  // namespace uu3d
