// uu3d_bones.h -- CONSTANT BONE LENGTHS (include/uu3d.h; predict.bone_lengths / fix_bones, predict.predict_tracks(bones=...),
// stream.StreamSession(bones=...)): every frame's skeleton is rebuilt from the tree root outwards with each bone scaled to ONE length per
// track (or slot), so a person's bones are rigid over time and the directions of the network's bones are kept.
//     bone_lengths_kernel        offline: one lane per (track, joint) walks the track's rows in order and averages the bone's length --
//                                adjacent lanes are adjacent joints of one row (the layout of one_euro_tracks_kernel)
//     fix_bones_kernel           offline: one lane per (row, joint) accumulates its own path from the root; a bone's scale is recomputed by
//                                every lane whose path crosses it, so no lane keeps an array of partial positions: no scratch memory
//     stream_bones_kernel        live: one wave per slot, lane j owns joint j -- the running mean of the fresh poses, then the fix
//     stream_bones_reset_kernel  chosen slots: sums and counts back to zero
// The rule is predict.bone_lengths_host's and predict.fix_bones_host's, statement for statement, in float64 with every operation rounded
// once (no fused multiply-add, IEEE square root and division): the device equals the numpy mirrors bit for bit.  Every output and state
// element has one writer, no atomics, the caller's buffers are only read: bitwise repeatable, capturable.
#pragma once
#include "uu3d_smooth.h"

namespace uu3d {

static constexpr int kBonesMaxJoints = 64;                              // J beyond it: UU3D_ERR_UNSUPPORTED (one wave per slot, live)
static constexpr int kBonesLanes = 64;

// a joint with a bone above it: its parent is another joint of the row (the tree root has -1; anything out of range counts as no bone)
__device__ __forceinline__ bool bone_parent_ok(const int j, const int p, const int J)
{
    return p >= 0 && p < J && p != j;
}

// The bone above joint j of one row (J, 3): d = x[j] - x[p] per coordinate, len = sqrt((d0 d0 + d1 d1) + d2 d2), the square root
// correctly rounded (numpy's is).
__device__ __forceinline__ double bone_offset(const float* __restrict__ row, const int j, const int p, double& d0, double& d1, double& d2)
{
#pragma clang fp contract(off)
    d0 = (double)row[j * 3 + 0] - (double)row[p * 3 + 0];
    d1 = (double)row[j * 3 + 1] - (double)row[p * 3 + 1];
    d2 = (double)row[j * 3 + 2] - (double)row[p * 3 + 2];
    return sqrt((d0 * d0 + d1 * d1) + d2 * d2);                          // (f64 sqrt of a build without fast-math: IEEE, rounded to nearest)
}

__device__ __forceinline__ bool bone_length_ok(const double v) { return finite_double(v) && v > 0.0; }

// poses (rows, J, 3) f32; parents (J) i32; track_start, track_len (tracks) i64: the rows of a track; lengths (tracks, J) f64; counts
// (tracks, J) i64 or nullptr.  Grid (tracks, ceil(J / 64)): the wave walks ONE track, so its trip count is uniform.  Every (track, joint)
// is written: the mean over the rows where the bone's length is finite and > 0, NaN where there is none, 0 for a joint without a bone.
static __global__ void __launch_bounds__(kBonesLanes)
bone_lengths_kernel(const float* __restrict__ poses, const long rows, const int J, const int32_t* __restrict__ parents,
                    const int64_t* __restrict__ track_start, const int64_t* __restrict__ track_len, double* __restrict__ lengths,
                    int64_t* __restrict__ counts)
{
#pragma clang fp contract(off)
    const int j = blockIdx.y * kBonesLanes + threadIdx.x;
    if (j >= J) return;
    const int track = blockIdx.x;
    const int p = parents[j];
    const bool bone = bone_parent_ok(j, p, J);
    long first = track_start[track], n = track_len[track];
    if (first < 0 || n < 1 || first >= rows) n = 0;
    else if (n > rows - first) n = rows - first;                         // (nothing is read beyond the buffer)
    double sum = 0.0;
    long count = 0;
    if (bone) {
        const float* row = poses + first * J * 3;
        for (long i = 0; i < n; ++i, row += J * 3) {
            double d0, d1, d2;
            const double len = bone_offset(row, j, p, d0, d1, d2);
            if (bone_length_ok(len)) {
                sum = sum + len;
                ++count;
            }
        }
    }
    const long e = (long)track * J + j;
    lengths[e] = !bone ? 0.0 : (count > 0 ? sum / (double)count : __longlong_as_double(0x7ff8000000000000LL));
    if (counts != nullptr) counts[e] = count;
}

// The position of joint j of one row with the bones on its path scaled: acc = x[root], then per joint a of the path, root side first,
// acc = acc + d(a) * s(a), s(a) = L[a] / len(a) where both are finite and > 0, else 1.  path: up to `depth` joints, -1 behind the last one;
// L: the lengths of the row's track, or nullptr (nothing is corrected).  An entry out of range ends the walk: nothing is read out of bounds.
__device__ __forceinline__ void bone_path_position(const float* __restrict__ row, const int J, const int32_t* __restrict__ parents,
                                                   const int32_t* __restrict__ path, const int depth, const double* __restrict__ L, const int j,
                                                   float& y0, float& y1, float& y2)
{
#pragma clang fp contract(off)
    y0 = row[j * 3 + 0];
    y1 = row[j * 3 + 1];
    y2 = row[j * 3 + 2];
    if (!bone_parent_ok(j, parents[j], J) || depth < 1) return;          // the tree root: the input bits
    const int first = path[0];
    if (first < 0 || first >= J || !bone_parent_ok(first, parents[first], J)) return;
    const int root = parents[first];
    double a0 = (double)row[root * 3 + 0], a1 = (double)row[root * 3 + 1], a2 = (double)row[root * 3 + 2];
    for (int k = 0; k < depth; ++k) {
        const int a = path[k];
        if (a < 0 || a >= J) break;
        const int p = parents[a];
        if (!bone_parent_ok(a, p, J)) break;
        double d0, d1, d2;
        const double len = bone_offset(row, a, p, d0, d1, d2);
        double s = 1.0;
        if (L != nullptr) {
            const double want = L[a];
            if (bone_length_ok(want) && bone_length_ok(len)) s = want / len;
        }
        a0 = a0 + d0 * s;
        a1 = a1 + d1 * s;
        a2 = a2 + d2 * s;
    }
    y0 = (float)a0;
    y1 = (float)a1;
    y2 = (float)a2;
}

// in, out (rows, J, 3) f32, out != in; parents (J) i32; paths (J, depth) i32; row_track (rows) i32 or nullptr (track 0); lengths
// (tracks, J) f64.  One lane per (row, joint); a row whose track is out of range is rebuilt with nothing corrected.
static __global__ void __launch_bounds__(256)
fix_bones_kernel(const float* __restrict__ in, float* __restrict__ out, const long rows, const int J, const int32_t* __restrict__ parents,
                 const int32_t* __restrict__ paths, const int depth, const int32_t* __restrict__ row_track, const int num_tracks,
                 const double* __restrict__ lengths)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * J) return;
    const long r = e / J;
    const int j = (int)(e - r * J);
    const int t = row_track == nullptr ? 0 : row_track[r];
    const double* L = (t >= 0 && t < num_tracks) ? lengths + (long)t * J : nullptr;
    float y0, y1, y2;
    bone_path_position(in + r * J * 3, J, parents, paths + (long)j * depth, depth, L, j, y0, y1, y2);
    float* dst = out + e * 3;
    dst[0] = y0;
    dst[1] = y1;
    dst[2] = y2;
}

// The state block of a live session, per slot and joint: the sum of the bone's lengths (f64) and how many were added (i32).
struct BonesLayout {
    size_t off_sum, off_count, bytes;
};
inline BonesLayout bones_layout(const int slots, const int J)
{
    BonesLayout L{};
    const size_t e = (size_t)slots * (size_t)J;
    L.off_sum = 0;
    L.off_count = one_euro_align(e * sizeof(double));
    L.bytes = L.off_count + one_euro_align(e * sizeof(int32_t));
    return L;
}

// One wave per slot, lane j owns joint j (J <= 64).  poses (T, J, 3) f32: what the tick emitted, only read; given (T, J) f64 or nullptr.
//   given == nullptr: an active slot whose pose is fresh first adds the finite, positive length of bone j to the slot's sum and counts it;
//       L[j] = sum / count (NaN before the first one, 0 for a joint without a bone).  The mean is CAUSAL: the poses seen so far.
//   given != nullptr: L[j] = given[slot][j] as it is; the state is not touched.
// Then EVERY slot, fresh or not, writes out = the pose rebuilt with L (bone_path_position): a pure function of the raw pose and the
// slot's lengths, so a slot that holds its previous raw pose returns its previous fixed pose, bit for bit.
static __global__ void __launch_bounds__(kBonesLanes)
stream_bones_kernel(const int J, const int32_t* __restrict__ parents, const int32_t* __restrict__ paths, const int depth,
                    const uint8_t* __restrict__ active, const uint8_t* __restrict__ fresh, const float* __restrict__ poses,
                    const double* __restrict__ given, double* __restrict__ sums, int32_t* __restrict__ counts, float* __restrict__ out,
                    double* __restrict__ lengths_out)
{
#pragma clang fp contract(off)
    __shared__ double L[kBonesLanes];
    const int slot = blockIdx.x, j = threadIdx.x;
    const float* row = poses + (long)slot * J * 3;
    if (j < J) {
        const long e = (long)slot * J + j;
        const int p = parents[j];
        const bool bone = bone_parent_ok(j, p, J);
        double want;
        if (given != nullptr) want = given[e];
        else {
            double sum = sums[e];
            int32_t count = counts[e];
            if (bone && active[slot] != 0 && fresh[slot] != 0) {
                double d0, d1, d2;
                const double len = bone_offset(row, j, p, d0, d1, d2);
                if (bone_length_ok(len)) {
                    sum = sum + len;
                    ++count;
                    sums[e] = sum;
                    counts[e] = count;
                }
            }
            want = !bone ? 0.0 : (count > 0 ? sum / (double)count : __longlong_as_double(0x7ff8000000000000LL));
        }
        L[j] = want;
        if (lengths_out != nullptr) lengths_out[e] = want;
    }
    __syncthreads();
    if (j < J) {
        float y0, y1, y2;
        bone_path_position(row, J, parents, paths + (long)j * depth, depth, L, j, y0, y1, y2);
        float* dst = out + ((long)slot * J + j) * 3;
        dst[0] = y0;
        dst[1] = y1;
        dst[2] = y2;
    }
}

// slot_mask (T) u8 or nullptr (every slot): the chosen slots have seen no pose.  One wave per slot.
static __global__ void __launch_bounds__(kBonesLanes)
stream_bones_reset_kernel(const uint8_t* __restrict__ slot_mask, const int J, double* __restrict__ sums, int32_t* __restrict__ counts)
{
    const int slot = blockIdx.x, j = threadIdx.x;
    if (j >= J || (slot_mask != nullptr && slot_mask[slot] == 0)) return;
    sums[(long)slot * J + j] = 0.0;
    counts[(long)slot * J + j] = 0;
}

}  // namespace uu3d
