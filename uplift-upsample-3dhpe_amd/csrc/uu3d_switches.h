// uu3d_switches.h -- every UU3D_* environment variable the library reads, in two structs by lifetime (INTEGRATION.md section 5
// lists them in this order).  No other file of the library calls getenv.  All of them are A/B and measurement switches: the
// defaults are the product path.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <string>

namespace uu3d {

// PER HANDLE: read by uu3d_create (a process can hold handles with different settings; the tests build two and compare).  The
// `train` part is read AGAIN by the handle's first uu3d_train_init, which is where the training step took them from the environment.
struct Switches {
    // UU3D_SPATIAL=f32 | h3 | h3tiles (anything else: by launch size, on spatial_stack_p16_kernel)
    bool spatial_f32 = false;         // f32: exact-f32 MFMA spatial stack even in f16x3 mode
    bool spatial_h3_always = false;   // h3: f16x3 spatial stack for every launch size
    bool spatial_h3_tiles = false;    // h3tiles: inference on the 32-token-tile kernel spatial_stack_h3_kernel
    bool no_planes = false;           // UU3D_NO_PLANES=1: keep the on-the-fly split GEMMs in f16x3 mode
    bool attn_wg = false;             // UU3D_ATTN_WG=1: attention with one workgroup per (sequence, head) (attn_f32_kernel) instead of one wave per item
    bool no_mlpf = false;             // UU3D_NO_MLPF=1: fc1 and fc2 of the temporal blocks as two GEMM launches
    bool no_wt = false;               // UU3D_NO_WT=1: few-row GEMMs stay on the tiled split-K kernels
    bool attn_f32 = false;            // UU3D_ATTN_F32=1: sequences of 49-128 tokens stay on the exact-f32 attention kernels
    bool no_panel = false;            // UU3D_NO_PANEL=1: LayerNorm-fed GEMMs stay on the tiled kernels
    bool no_panel_proj = false;       // UU3D_NO_PANEL_PROJ=1: the attention projection stays on the tiled LDS-DMA kernel
    // When the temporal chain (uu3d_tchain16.h) runs: under the throughput schedule, whenever the shapes allow it (>= 1024 token rows, attention
    // on attn_h3_kernel, no attention maps asked for).
    // History: round 5 (128-row tiles, residual adds as float atomics, profiles/r05_tchain_ab.txt) 179-187 k sequences/s against 171-175 k of the round-4
    // launches at batch 128; round 6 (64-row tiles, everything on chip, profiles/r06_ab_tchain16.txt) 197-212 k on the same box as 179-201 k.
    int tchain_mode = -1;             // UU3D_TCHAIN=0 | 1: -1 by size (tchain_min_tiles), 0 never (the round-4 launches), 1 always
    int tchain_min_tiles = 8;         // UU3D_TCHAIN_MIN_TILES=n: at least n 128-row tiles (default = the 1024 rows the panel kernels ask for as well)
    bool tchain_short = true;         // UU3D_TCHAIN_SHORT=0: the chain only where attn_h3_kernel is the attention kernel anyway.  Default: also below 49 tokens, on
                                      // attn_h3_kernel reading the chain's fragment-ordered q | k | v (h36m_81, batch 256: 337 k -> 361 k sequences/s)
    struct Train {                    // (presence switches: any value, the empty string too)
        bool f32 = false;             // UU3D_TRAIN_F32: every training GEMM exact f32 (no f16 operand planes)
        bool one_stream = false;      // UU3D_TRAIN_1STREAM: the parameter-gradient work in order on the caller's stream
        bool event_flags_set = false; // UU3D_TRAIN_EVENT_FLAGS=<int>: the extra hipEventCreateWithFlags bits of the cross-stream events
        unsigned event_flags = 0;     //   (unset: hipEventReleaseToDevice)
        bool any_queue = false;       // UU3D_TRAIN_ANY_QUEUE: the first side streams HIP hands out, no probing for hardware queues of their own
        bool spatial_unfused = false; // UU3D_TRAIN_SPATIAL_UNFUSED: the spatial stack's training forward as the chain of generic kernels
        bool no_panel = false;        // UU3D_TRAIN_NO_PANEL: LayerNorm-fed Dense layers on row_stats + the tiled GEMM
        bool attn_bwd_generic = false;// UU3D_ATTN_BWD_GENERIC: every attention backward on the generic kernel (the ops ABI, which has no handle, reads it per call)
    } train;
};

inline Switches read_switches() {
    Switches s;
    auto is1 = [](const char* name) { const char* e = getenv(name); return e != nullptr && e[0] == '1'; };
    auto present = [](const char* name) { return getenv(name) != nullptr; };
    { const char* e = getenv("UU3D_SPATIAL"); const std::string v = e ? e : "";
      s.spatial_f32 = v == "f32"; s.spatial_h3_always = v == "h3"; s.spatial_h3_tiles = v == "h3tiles"; }
    s.no_planes = is1("UU3D_NO_PLANES");
    s.attn_wg = is1("UU3D_ATTN_WG");
    s.no_mlpf = is1("UU3D_NO_MLPF");
    s.no_wt = is1("UU3D_NO_WT");
    s.attn_f32 = is1("UU3D_ATTN_F32");
    s.no_panel = is1("UU3D_NO_PANEL");
    s.no_panel_proj = is1("UU3D_NO_PANEL_PROJ");
    { const char* e = getenv("UU3D_TCHAIN"); if (e != nullptr && (e[0] == '0' || e[0] == '1')) s.tchain_mode = e[0] - '0'; }
    { const char* e = getenv("UU3D_TCHAIN_MIN_TILES"); if (e != nullptr && atoi(e) > 0) s.tchain_min_tiles = atoi(e); }
    { const char* e = getenv("UU3D_TCHAIN_SHORT"); if (e != nullptr) s.tchain_short = atoi(e) != 0; }
    s.train.f32 = present("UU3D_TRAIN_F32");
    s.train.one_stream = present("UU3D_TRAIN_1STREAM");
    { const char* e = getenv("UU3D_TRAIN_EVENT_FLAGS"); s.train.event_flags_set = e != nullptr; if (e) s.train.event_flags = (unsigned)strtoul(e, nullptr, 0); }
    s.train.any_queue = present("UU3D_TRAIN_ANY_QUEUE");
    s.train.spatial_unfused = present("UU3D_TRAIN_SPATIAL_UNFUSED");
    s.train.no_panel = present("UU3D_TRAIN_NO_PANEL");
    s.train.attn_bwd_generic = present("UU3D_ATTN_BWD_GENERIC");
    return s;
}

// PER PROCESS: read once, at the first use of any of them; later changes of the environment are not seen.
struct ProcessSwitches {
#ifdef UU3D_TIMING_BUILD              // (timing builds only -- build.py --timing: the product library does not contain the names)
    // UU3D_SKIP=<bit mask> (TIMING EXPERIMENTS ONLY: the skipped launches leave garbage, results are wrong): which launch classes of the
    // forward are left out -- 1 spatial stack, 2 LayerNorm-fed panel GEMMs (QKV, fc1), 4 projection, 8 fused MLP, 16 attention, 32 ln_split_frag,
    // 64 ln_res_split_frag, 128 the temporal chain launches, 256 strided blocks 2.., 512 strided block 1.  tools/marginal_exp.sh prices what each
    // class costs the pipelined step.
    int skip = 0;
    bool timing_parts = false;        // UU3D_TIMING_PARTS=1: the schedule bits 0x200 / 0x400 (tools/tail_branch_exp.py) are honoured
#endif
    bool panel4 = false;              // UU3D_PANEL4=1: every row-panel GEMM on the 4-wave kernel
    int panel_s = 0;                  // UU3D_PANEL_S=1|2|3: column ranges per row tile of the row-panel GEMMs (0: by the cost model)
    int panel_proj_s = 0;             // UU3D_PANEL_PROJ_S=1|2|3: the same for the attention projection
    bool no_ln_tail = false;          // UU3D_NO_LN_TAIL (presence): LayerNorm 2 never rides in the projection's launch
    int thr_splitk_target = 192;      // UU3D_THR_SPLITK_TARGET=n: workgroups a split-K GEMM beside the temporal chain aims for
    int tnh_wgs = 192;                // UU3D_TNH_WGS=n: workgroup target of the weight-gradient split (training)
    int gemm_deep_wgs = 640;          // UU3D_GEMM_DEEP_WGS=n: tiled f16x3 GEMM launches of at most n workgroups load three k-tiles ahead (0: never)
    bool tn_f32 = false;              // UU3D_TN_F32 (presence): weight-gradient GEMMs on the exact-f32 kernel
    bool capture_inorder = false;     // UU3D_TRAIN_CAPTURE_INORDER (presence): a captured training step stays on the caller's stream
};

inline const ProcessSwitches& process_switches() {
    static const ProcessSwitches sw = [] {
        ProcessSwitches s;
#ifdef UU3D_TIMING_BUILD
        { const char* e = getenv("UU3D_SKIP"); s.skip = e ? atoi(e) : 0;
          if (s.skip) fprintf(stderr, "[uu3d] UU3D_SKIP=%d: launches are being skipped, RESULTS ARE WRONG (timing experiment)\n", s.skip); }
        { const char* e = getenv("UU3D_TIMING_PARTS"); s.timing_parts = e != nullptr && atoi(e) != 0; }
#endif
        { const char* e = getenv("UU3D_PANEL4"); s.panel4 = e != nullptr && atoi(e) != 0; }
        { const char* e = getenv("UU3D_PANEL_S"); if (e != nullptr && e[0] >= '1' && e[0] <= '3') s.panel_s = e[0] - '0'; }
        { const char* e = getenv("UU3D_PANEL_PROJ_S"); if (e != nullptr && e[0] >= '1' && e[0] <= '3') s.panel_proj_s = e[0] - '0'; }
        s.no_ln_tail = getenv("UU3D_NO_LN_TAIL") != nullptr;
        { const char* e = getenv("UU3D_THR_SPLITK_TARGET"); if (e != nullptr && atoi(e) > 0) s.thr_splitk_target = atoi(e); }
        { const char* e = getenv("UU3D_TNH_WGS"); if (e != nullptr) s.tnh_wgs = atoi(e); }
        { const char* e = getenv("UU3D_GEMM_DEEP_WGS"); if (e != nullptr) s.gemm_deep_wgs = atoi(e); }
        s.tn_f32 = getenv("UU3D_TN_F32") != nullptr;
        s.capture_inorder = getenv("UU3D_TRAIN_CAPTURE_INORDER") != nullptr;
        return s;
    }();
    return sw;
}

}  // namespace uu3d
