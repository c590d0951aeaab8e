// path_pending_check.cpp -- host program (own main) for pp2_path_pending.h,
// the context's list of what changed since the shortest-path field was solved
// (pp2_map_update and pp2_goal_set write it, pp2_path_resolve reads it): built
// and run by tests/test_path_resolve_cpu.py with the host compiler.
//
// Cases: a fresh list is empty and allows a warm re-solve only under the goal
// state it was cleared with; boxes are stored as rectangles in order, with
// their free-to-occupied bit; an empty box adds nothing; the 17th box sets
// the overflow flag, writes nothing past the array and stays set until
// clear(); the goal flag and a changed goal cell each refuse the warm path;
// cells() sums the areas; clear() resets everything.
#include <stdio.h>

#include "pp2_path_pending.h"

using pp2::kPathPendingCap;
using pp2::PathPending;
using pp2::PathRect;

static int failures = 0;

#define EXPECT(cond)                                            \
  do {                                                          \
    if (!(cond)) {                                              \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++failures;                                               \
    }                                                           \
  } while (0)

static bool same(const PathRect& a, int x0, int y0, int w, int h, int raised) {
  return a.x0 == x0 && a.y0 == y0 && a.w == w && a.h == h && a.raised == raised;
}

// the list between two guards: add() writes r[0 .. n) and nothing else
struct Guarded {
  int before[8];
  PathPending p;
  int after[8];
  Guarded() {
    for (int& v : before) v = 0x5a5a5a5a;
    for (int& v : after) v = 0x5a5a5a5a;
  }
  bool intact() const {
    for (int v : before)
      if (v != 0x5a5a5a5a) return false;
    for (int v : after)
      if (v != 0x5a5a5a5a) return false;
    return true;
  }
};

int main() {
  {  // fresh
    PathPending p;
    EXPECT(p.empty() && p.n == 0 && !p.overflow && !p.goal_moved && !p.goal_free);
    EXPECT(p.warm_ok(false) && !p.warm_ok(true));
    EXPECT(!p.any_raised() && p.cells() == 0);
    p.clear(true);
    EXPECT(p.empty() && p.goal_free && p.warm_ok(true) && !p.warm_ok(false));
  }
  {  // boxes in order, inclusive corners to rectangles
    PathPending p;
    p.clear(true);
    p.add(3, 4, 3, 4, true);
    p.add(0, 0, 9, 1, false);
    p.add(5, 7, 6, 9, false);
    EXPECT(p.n == 3 && !p.empty() && !p.overflow);
    EXPECT(same(p.r[0], 3, 4, 1, 1, 1));
    EXPECT(same(p.r[1], 0, 0, 10, 2, 0));
    EXPECT(same(p.r[2], 5, 7, 2, 3, 0));
    EXPECT(p.cells() == 1 + 20 + 6);
    EXPECT(p.any_raised() && p.warm_ok(true));
    // an update that changed no occupancy: its box is empty
    p.add(10, 0, -1, -1, false);
    p.add(0, 10, 5, 9, true);
    EXPECT(p.n == 3 && !p.overflow);
  }
  {  // freed-only rectangles: nothing to raise
    PathPending p;
    for (int i = 0; i < 5; ++i) p.add(i, i, i + 2, i + 1, false);
    EXPECT(p.n == 5 && !p.any_raised() && p.cells() == 5 * 6);
    p.add(9, 9, 9, 9, true);
    EXPECT(p.any_raised());
  }
  {  // capacity, overflow
    Guarded g;
    PathPending& p = g.p;
    p.clear(true);
    for (int i = 0; i < kPathPendingCap; ++i) p.add(i, 2 * i, i, 2 * i, i % 2 == 0);
    EXPECT(p.n == kPathPendingCap && !p.overflow && p.warm_ok(true));
    for (int i = 0; i < kPathPendingCap; ++i) EXPECT(same(p.r[i], i, 2 * i, 1, 1, i % 2 == 0));
    p.add(100, 100, 101, 101, true);
    EXPECT(p.n == kPathPendingCap && p.overflow && !p.warm_ok(true) && !p.empty());
    for (int i = 0; i < 3 * kPathPendingCap; ++i) p.add(i, i, i, i, false);
    EXPECT(p.n == kPathPendingCap && p.overflow);
    for (int i = 0; i < kPathPendingCap; ++i) EXPECT(same(p.r[i], i, 2 * i, 1, 1, i % 2 == 0));
    EXPECT(g.intact());
    p.clear(true);
    EXPECT(p.empty() && p.n == 0 && !p.overflow && p.warm_ok(true));
    p.add(1, 1, 1, 1, false);
    EXPECT(p.n == 1 && same(p.r[0], 1, 1, 1, 1, 0));
    EXPECT(g.intact());
  }
  {  // the goal
    PathPending p;
    p.clear(true);
    p.goal_moved = true;
    EXPECT(!p.empty() && !p.warm_ok(true) && !p.warm_ok(false));
    p.clear(false);
    EXPECT(p.empty() && !p.goal_moved && p.warm_ok(false) && !p.warm_ok(true));
    // the goal cell occupied and freed again between two re-solves: as before
    p.clear(true);
    p.add(2, 2, 2, 2, true);
    p.add(2, 2, 2, 2, false);
    EXPECT(p.n == 2 && p.warm_ok(true) && !p.warm_ok(false));
  }
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("pending capacity %d: all cases hold\n", kPathPendingCap);
  return 0;
}
