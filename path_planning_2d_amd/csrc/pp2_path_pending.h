// pp2_path_pending.h -- private, plain host code: what changed since the
// shortest-path field in the planes was solved (pp2_path_resolve; DESIGN.md
// §2.3 "Warm re-solve").  pp2_map_update appends the bounding box of the cells
// whose occupancy it changed, and whether any of them went from free to
// occupied; pp2_goal_set notes that the goal moved.  A warm re-solve visits
// the cells of the rectangles alone and compares the map in force with the
// field, so a cell changed twice needs no bookkeeping and rectangles may
// overlap.  A fixed list: once it is full the answer is "unknown" and the
// re-solve starts cold.  The model journal (pp2_journal.h) cannot serve here:
// it records only while a model exists, and the field needs none.  No HIP
// here, so that tests/path_pending_check.cpp builds it with the host compiler.
#pragma once

namespace pp2 {

constexpr int kPathPendingCap = 16;  // rectangles the list holds

struct PathRect {
  int x0, y0, w, h;  // cells [x0, x0 + w) x [y0, y0 + h), non-empty
  int raised;        // 1: some cell of it went from free to occupied
};

struct PathPending {
  PathRect r[kPathPendingCap];
  int n = 0;
  bool overflow = false;    // an update found the list full: the changes are unknown
  bool goal_moved = false;  // pp2_goal_set since the field
  bool goal_free = false;   // the goal cell was on the grid and free at field time

  // a new field: nothing pending, the goal as it is now
  void clear(bool goal_free_now = false) {
    n = 0;
    overflow = goal_moved = false;
    goal_free = goal_free_now;
  }

  // The inclusive box [bx0, bx1] x [by0, by1] of one update; an empty box
  // (bx1 < bx0 or by1 < by0) is no change.
  void add(int bx0, int by0, int bx1, int by1, bool raised) {
    if (bx1 < bx0 || by1 < by0) return;
    if (n == kPathPendingCap) {
      overflow = true;
      return;
    }
    r[n++] = PathRect{bx0, by0, bx1 - bx0 + 1, by1 - by0 + 1, raised ? 1 : 0};
  }

  bool empty() const { return n == 0 && !overflow && !goal_moved; }
  // the rectangles say everything that changed, and the goal stands as it did
  bool warm_ok(bool goal_free_now) const {
    return !overflow && !goal_moved && goal_free_now == goal_free;
  }
  bool any_raised() const {
    for (int i = 0; i < n; ++i)
      if (r[i].raised) return true;
    return false;
  }
  long long cells() const {  // overlaps count once per rectangle
    long long c = 0;
    for (int i = 0; i < n; ++i) c += (long long)r[i].w * r[i].h;
    return c;
  }
};

}  // namespace pp2
