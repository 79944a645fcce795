// The key-frame decision chain of modules/videostrip/src/main.cpp:284-394 (first frame = key frame; a frame whose overlap
// with the key frame is <= minOverlap, -2.0 counted as OVERLAP_MIN + 0.01 (:321-329), opens a window: the sharpest of it
// and the next kWindow frames by calcBlur becomes the new key frame, :335-381), written ONCE for two back ends:
//   k_kf_chain (kf_chain.hip)      one lane on the device, behind the matcher launches of a pipe step;
//   uwip_keyframe_chain_host       the host, with the overlaps / blurs supplied by callbacks (the CPU tests).
// The walker only READS overlaps that are already known.  They come from pair lists matched ahead of it:
//   round 0      a fixed list: (i, key slot 0) and (i, i - d), d = 1..D, for every frame i of the batch;
//   rounds 1..R  one list per round, written by the walker when it needs an overlap that no earlier list holds: every
//                batch frame from that one on against the current key (the walker stops there and resumes after the
//                matcher has run on the list).
// Feature slots of a pipe in key-frame mode (F = frames per batch):  0 = the current key frame at the start of a batch,
// 1..F = this batch's frames, F + 1 = the best candidate of a window that was open when the previous batch ended.
// The "Frame" column keeps the reference's numbering: a trigger frame that stays best reports its 0-based stream index
// (:340 reads it before the window), a window frame the 1-based count of frames read (:364).
#pragma once
#include <cmath>
#include <cstdint>
#include "../../include/uwip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KF_HD __host__ __device__
#else
#define KF_HD
#endif

namespace uwip_kf {

constexpr float OVERLAP_MIN = 0.4f;       // videostrip.hpp:50: what a -2.0 (no homography) counts as, + 0.01

// Chain state: lives in pipe-owned device memory (or on the host stack) and carries across batches.
struct State {
    int32_t key_slot, key_index;          // current key frame: feature slot and stream index
    int32_t nxt;                          // stream index of the next frame to read (the reference's `read` counter)
    int32_t win_left;                     // window frames still to scan; 0 = no window open
    int32_t best_slot, best_index, best_frame;
    float best_blur, trig_ov;             // best candidate's blur, the trigger's overlap (after -2.0 -> 0.41)
    int32_t next_id;                      // ID of the next row (restarts with a stream)
    uint32_t total;                       // rows written to the ring since the pipe was made (never restarts)
    int32_t err;                          // 1: a batch was not resolved within the round bound (until uwip_pipe_keyframes reports it)
    int32_t broken;                       // the chain stopped at that batch; the walker does nothing until a new stream starts
    int32_t done;                         // this batch has been walked to its end
    int32_t nfb;                          // fallback rounds requested in this batch
    int32_t carry_key, carry_best;        // slots the step's last kernel copies to slot 0 / slot F + 1 (-1: none)
};

// One batch: everything the host knows when it queues the step.
struct Batch {
    int32_t F, D, kWindow, valid, base, rounds, max_rows;
    float minOverlap;
    int32_t first, last;                  // first batch of a stream / last batch (end of stream after `valid` frames)
};

// Where the walker reads and writes.  out_ratio / out_info: the matcher's per-pair results, round 0's P0 pairs first,
// then F per fallback round.  fb_key / fb_start [rounds + 1]: key slot and first frame of each fallback round's list.
struct Bufs {
    const float *out_ratio;
    const int32_t *out_info;              // [pair][8]
    const float *blur;                    // [F] calcBlur of the resized batch frames
    float *ratio;                         // [F] the step's d_ratio
    int32_t *info;                        // [F][8] the step's d_info (may be null)
    uwip_keyframe_row *ring;              // [max_rows]
    int32_t *fb_key, *fb_start;
    int32_t *fb_q, *fb_t, *fb_n;          // the next round's pair list [F] + [F] and its length
};

KF_HD inline int eff_lookback(int F, int D) { return D < F - 1 ? D : F - 1; }

// pairs in round 0's list
KF_HD inline int round0_pairs(int F, int D)
{
    const int d = eff_lookback(F, D);
    return F * (d + 1) - d * (d + 1) / 2;
}

// Index of the pair (frame i, frame i - d) in round 0's list: (i, slot 0) for i = 0..F-1 first, then d = 1, 2, .. each for
// i = d..F-1.
KF_HD inline int round0_index(int F, int i, int d)
{
    return d == 0 ? i : F + (d - 1) * F - (d - 1) * d / 2 + (i - d);
}

// round 0's list, q / t [round0_pairs]: query slot 1 + i, train slot 0 (the key) or 1 + i - d
inline void round0_list(int F, int D, int32_t *q, int32_t *t)
{
    const int Dp = eff_lookback(F, D);
    for (int d = 0; d <= Dp; ++d)
        for (int i = d; i < F; ++i) {
            const int at = round0_index(F, i, d);
            q[at] = 1 + i;
            t[at] = d == 0 ? 0 : 1 + i - d;
        }
}

inline bool config_ok(const uwip_keyframe_config &kc)
{
    return !std::isnan(kc.minOverlap) && kc.kWindow >= 0 && kc.lookback >= 1 && kc.lookback <= 4096 && kc.max_rows >= 1 &&
           kc.max_rows <= (1 << 24);
}

// Fallback rounds a batch can need.  A miss is the first look-up of an overlap against a key that no earlier list holds;
// after a miss at frame m with key K, every later frame against K is in that round's list, so the next miss needs a new
// key: a trigger at some t >= m, then the window of kWindow frames, then the first comparison at t + kWindow + 1 >= m +
// kWindow + 1.  With kWindow = 0 the new key is the trigger t itself, and round 0 holds frames t + 1..t + D against it,
// so the next miss is at >= m + D + 1.  Misses at least s apart in F frames: at most (F - 1) / s + 1 of them.
KF_HD inline int max_rounds(int F, int D, int kWindow)
{
    const int s = kWindow > 0 ? kWindow + 1 : eff_lookback(F, D) + 1;
    return (F - 1) / s + 1;
}

KF_HD inline int lookup(const Batch &b, const State &s, const Bufs &u, int i)
{
    const int k = s.key_slot;
    if (k == 0) return i;
    const int d = i - (k - 1);
    if (k <= b.F && d >= 1 && d <= eff_lookback(b.F, b.D)) return round0_index(b.F, i, d);
    const int P0 = round0_pairs(b.F, b.D);
    for (int r = 1; r <= s.nfb; ++r)
        if (u.fb_key[r] == k && i >= u.fb_start[r]) return P0 + (r - 1) * b.F + (i - u.fb_start[r]);
    return -1;
}

KF_HD inline void emit(const Batch &b, State &s, const Bufs &u, int32_t id, int32_t frame, int32_t index, float ov, float blur)
{
    uwip_keyframe_row &r = u.ring[s.total % (uint32_t)b.max_rows];
    r.id = id; r.frame = frame; r.index = index; r.overlap = ov; r.blur = blur;
    r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
    s.total += 1;
}

// the window closes: its best candidate is the new key frame and its row is written (main.cpp:368-381)
KF_HD inline void close_window(const Batch &b, State &s, const Bufs &u)
{
    emit(b, s, u, s.next_id, s.best_frame, s.best_index, s.trig_ov, s.best_blur);
    s.next_id += 1;
    s.key_slot = s.best_slot;
    s.key_index = s.best_index;
    s.win_left = 0;
}

// One walker call: round `round` (0 = the first of the batch).  Walks as far as the known overlaps reach; returns with
// *u.fb_n = the length of the pair list the next round must match (0 = nothing more to do in this batch).
KF_HD inline void walk(const Batch &b, State &s, const Bufs &u, int round)
{
    const int F = b.F;
    if (round == 0) {
        if (b.first) {
            s.key_slot = 0;                     // the host has copied frame 0's features (slot 1) to slot 0
            s.key_index = b.base;
            s.nxt = b.base + 1;
            s.win_left = 0;
            s.next_id = 0;
            emit(b, s, u, 0, 0, b.base, 0.0f, 0.0f);     // main.cpp:297: the first frame's row
            s.next_id = 1;
            s.broken = 0;
        }
        s.done = 0;
        s.nfb = 0;
        s.carry_key = s.carry_best = -1;        // nothing to carry unless the batch is walked to its end
        for (int i = 0; i < F; ++i) {
            u.ratio[i] = NAN;
            if (u.info) {
                for (int f = 0; f < 8; ++f) u.info[8 * i + f] = 0;
                u.info[8 * i + 5] = -1;
            }
        }
    }
    *u.fb_n = 0;
    if (s.done || s.broken) return;
    const int end = b.base + b.valid;
    if (s.nxt < b.base) {                       // a stream position outside this batch: stop rather than index outside it
        s.err = s.broken = s.done = 1;
        return;
    }
    while (s.nxt < end) {
        const int i = s.nxt - b.base;
        if (s.win_left > 0) {                   // :344-366: blur only, no overlap
            const float bl = u.blur[i];
            if (bl > s.best_blur) {
                s.best_blur = bl;
                s.best_frame = s.nxt + 1;
                s.best_index = s.nxt;
                s.best_slot = 1 + i;
            }
            s.nxt += 1;
            if (--s.win_left == 0) close_window(b, s, u);
            continue;
        }
        const int p = lookup(b, s, u, i);
        if (p < 0) {
            if (s.nfb >= b.rounds) {            // cannot happen within the bound (max_rounds); reported, not walked past
                s.err = s.broken = s.done = 1;
                return;
            }
            s.nfb += 1;
            u.fb_key[s.nfb] = s.key_slot;
            u.fb_start[s.nfb] = i;
            for (int j = i; j < b.valid; ++j) { u.fb_q[j - i] = 1 + j; u.fb_t[j - i] = s.key_slot; }
            *u.fb_n = b.valid - i;
            return;
        }
        const float raw = u.out_ratio[p];
        u.ratio[i] = raw;
        if (u.info) {
            for (int f = 0; f < 5; ++f) u.info[8 * i + f] = u.out_info[8 * (size_t)p + f];
            u.info[8 * i + 5] = s.key_index;
        }
        s.nxt += 1;
        const float ov = raw == -2.0f ? OVERLAP_MIN + 0.01f : raw;
        if (ov <= b.minOverlap) {               // :329-340: the trigger is the first candidate
            s.best_blur = u.blur[i];
            s.best_frame = s.nxt - 1;
            s.best_index = s.nxt - 1;
            s.best_slot = 1 + i;
            s.trig_ov = ov;
            s.win_left = b.kWindow;
            if (b.kWindow == 0) close_window(b, s, u);
        }
    }
    s.done = 1;
    if (b.last) {
        if (s.win_left > 0) close_window(b, s, u);      // the stream ends inside a window: its best so far (B-14)
        s.carry_key = s.carry_best = -1;
    } else if (s.win_left > 0) {
        s.carry_key = -1;                       // the key is done with: the window's best will be the next one
        s.carry_best = s.best_slot != F + 1 ? s.best_slot : -1;
        s.best_slot = F + 1;
    } else {
        s.carry_key = s.key_slot != 0 ? s.key_slot : -1;
        s.carry_best = -1;
        s.key_slot = 0;
    }
}

}  // namespace uwip_kf
