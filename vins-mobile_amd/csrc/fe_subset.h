// fe_subset.h -- per-call planning of the front end's subset calls (vio_frontend_submit_subset / vio_frontend_reset): plain host
// C++, no HIP. A context's sequences each carry their own phase of FeatureTracker::readImage (feature_tracker.cpp:162-310):
//   have[s]  the sequence has seen a frame (cur_img is not empty, :165)
//   bank[s]  which of the context's two pyramid banks holds the sequence's cur image (0 while have[s] == 0)
// A call names n sequences; the plan says, per call position i, where the frame goes (the forw bank), what LK tracks from (the
// prev bank, or kNoPrev for a first frame: pre = cur = forw, :166-167), and which positions publish. It is written into one
// arena of 32-bit integers that travels to the device as it is; the phase bits change only when the plan is committed.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace fe_subset {

constexpr int32_t kNoPrev = -1;
constexpr int kArenaRows = 6;  // seq | slot | prev_bank | forw_bank | publish | pub, n entries each

struct Arena {
  int32_t *seq;        // [n] sequence of call position i
  int32_t *slot;       // [n] frame slot of call position i
  int32_t *prev_bank;  // [n] bank of the image LK tracks from, kNoPrev: first frame of the sequence
  int32_t *forw_bank;  // [n] bank the frame's pyramid is written to: the sequence's cur bank after the call
  int32_t *publish;    // [n] 0 / 1
  int32_t *pub;        // [n_pub] call positions that publish, ascending
};

inline size_t arena_ints(int n) { return (size_t)kArenaRows * (size_t)(n > 0 ? n : 0); }
inline Arena carve(int32_t *base, int n) {
  Arena A;
  A.seq = base, A.slot = base + n, A.prev_bank = base + 2 * (size_t)n, A.forw_bank = base + 3 * (size_t)n;
  A.publish = base + 4 * (size_t)n, A.pub = base + 5 * (size_t)n;
  return A;
}

// seq[0..n): every entry inside [0, n_seq), none twice. `seen` is n_seq bytes of scratch.
inline bool valid_list(int n_seq, int n, const int32_t *seq, uint8_t *seen) {
  if (n < 0 || n > n_seq || (n > 0 && !seq)) return false;
  for (int s = 0; s < n_seq; s++) seen[s] = 0;
  for (int i = 0; i < n; i++) {
    if (seq[i] < 0 || seq[i] >= n_seq || seen[seq[i]]) return false;
    seen[seq[i]] = 1;
  }
  return true;
}

// The plan of one call. frame_index: null = position i takes slot i; n_slots < 0: slots are not bounded above.
// Returns false for bad arguments; nothing is written to the phase bits either way (commit does that).
inline bool plan(int n_seq, const uint8_t *bank, const uint8_t *have, int n, const int32_t *seq, const int32_t *frame_index,
                 int n_slots, const uint8_t *publish, uint8_t *seen, Arena A, int *n_pub) {
  if (!valid_list(n_seq, n, seq, seen) || (n > 0 && !publish)) return false;
  for (int i = 0; i < n && frame_index; i++)
    if (frame_index[i] < 0 || (n_slots >= 0 && frame_index[i] >= n_slots)) return false;
  int np = 0;
  for (int i = 0; i < n; i++) {
    const int s = seq[i];
    A.seq[i] = s, A.slot[i] = frame_index ? frame_index[i] : i;
    A.prev_bank[i] = have[s] ? (int32_t)bank[s] : kNoPrev;
    A.forw_bank[i] = have[s] ? 1 - (int32_t)bank[s] : (int32_t)bank[s];
    A.publish[i] = publish[i] ? 1 : 0;
    if (publish[i]) A.pub[np++] = i;
  }
  *n_pub = np;
  return true;
}

// cur_img = forw_img (:284) for the called sequences
inline void commit(uint8_t *bank, uint8_t *have, int n, const Arena &A) {
  for (int i = 0; i < n; i++) bank[A.seq[i]] = (uint8_t)A.forw_bank[i], have[A.seq[i]] = 1;
}

// a fresh FeatureTracker for the listed sequences (seq null: all of them)
inline void reset(int n_seq, uint8_t *bank, uint8_t *have, int n, const int32_t *seq) {
  if (!seq)
    for (int s = 0; s < n_seq; s++) bank[s] = have[s] = 0;
  else
    for (int i = 0; i < n; i++) bank[seq[i]] = have[seq[i]] = 0;
}

// every sequence in the same phase: what the lock-step entry points need
inline bool in_step(int n_seq, const uint8_t *bank, const uint8_t *have) {
  for (int s = 1; s < n_seq; s++)
    if (bank[s] != bank[0] || have[s] != have[0]) return false;
  return true;
}

}  // namespace fe_subset
