// pp2_journal.h -- private, plain host code: the context's journal of model
// updates (pp2_map_update, pp2_goal_set).  model_follow records
// the two clipped rectangles whose cells it regenerated together with the
// model_serial they produced; an object that cached model data at an older
// serial (the planner, pp2_planner_refresh) asks for the rectangles of every
// update since and patches those cells alone.  A fixed ring: once it no longer
// reaches back to the asked serial the answer is "unknown" and the asker
// refreshes in full.  No HIP here, so that tests/planner_journal_check.cpp
// builds it with the host compiler.
#pragma once

namespace pp2 {

constexpr int kJournalCap = 16;  // updates the ring remembers

struct JournalRect {
  int x0, y0, w, h;  // as PatchRect (pp2_internal.h); w or h of 0: none
};

struct ModelJournal {
  struct Entry {
    unsigned serial;  // the model_serial this update produced
    JournalRect r[2];
  };
  Entry e[kJournalCap];
  int head = 0;   // the slot the next record takes
  int count = 0;  // valid entries, <= kJournalCap

  void clear() { head = count = 0; }

  void record(unsigned serial, JournalRect r0, JournalRect r1) {
    e[head].serial = serial;
    e[head].r[0] = r0;
    e[head].r[1] = r1;
    head = (head + 1) % kJournalCap;
    if (count < kJournalCap) ++count;
  }
};

// The non-empty rectangles of every update newer than `since`, oldest first,
// into rects[0 .. *n) (room for 2 * kJournalCap), given the serial `current`
// of the model in force.  Serials advance by one per update (unsigned, so a
// wrap-around of the counter is harmless).  Returns false -- unknown -- when
// the ring does not hold every one of those updates: more than kJournalCap of
// them, a `since` ahead of `current`, or a gap in the recorded serials (an
// update that was not journalled).  since == current: true with *n = 0.
inline bool journal_changes_since(const ModelJournal& j, unsigned current, unsigned since,
                                  JournalRect* rects, int* n) {
  *n = 0;
  const unsigned k = current - since;  // updates asked for
  if (k == 0) return true;
  if (k > (unsigned)j.count) return false;
  int out = 0;
  for (unsigned i = 0; i < k; ++i) {
    // the i-th oldest of the last k records
    const int slot = (j.head - (int)k + (int)i + 2 * kJournalCap) % kJournalCap;
    const ModelJournal::Entry& en = j.e[slot];
    if (en.serial != since + 1 + i) return false;
    for (const JournalRect& r : en.r)
      if (r.w > 0 && r.h > 0) rects[out++] = r;
  }
  *n = out;
  return true;
}

// Cells of n rectangles (overlaps count once per rectangle).
inline long long journal_cells(const JournalRect* rects, int n) {
  long long c = 0;
  for (int i = 0; i < n; ++i) c += (long long)rects[i].w * rects[i].h;
  return c;
}

}  // namespace pp2
