// planner_journal_check.cpp -- host program (own main) for pp2_journal.h, the
// context's ring of model updates that pp2_planner_refresh reads: built and
// run by tests/test_planner_refresh_cpu.py with the host compiler.
//
// Cases: a serial equal to the current one gives no rectangles; k updates back
// gives those k rectangle pairs, oldest first, empty rectangles dropped;
// capacity + 1 back is unknown; the ring wraps (three times its capacity of
// updates, asked at every distance after each); a serial ahead of the current
// one and a gap in the recorded serials are unknown; the serial counter may
// wrap around 2^32.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pp2_journal.h"

using pp2::JournalRect;
using pp2::kJournalCap;
using pp2::ModelJournal;

static int failures = 0;

#define EXPECT(cond)                                            \
  do {                                                          \
    if (!(cond)) {                                              \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++failures;                                               \
    }                                                           \
  } while (0)

// The rectangles update number i (1-based) records: the first always, the
// second on every third update (a goal move has two, a map patch one).
static JournalRect first_of(unsigned i) { return JournalRect{(int)i, (int)(2 * i), 1 + (int)(i % 5), 1 + (int)(i % 3)}; }
static JournalRect second_of(unsigned i) {
  if (i % 3 != 0) return JournalRect{0, 0, 0, 0};
  return JournalRect{(int)(7 * i), (int)i, 1, 1};
}

static bool same(const JournalRect& a, const JournalRect& b) {
  return a.x0 == b.x0 && a.y0 == b.y0 && a.w == b.w && a.h == b.h;
}

// After `done` updates on a context whose serial started at `start`: ask at
// every distance 0 .. kJournalCap + 2.
static void ask_all(const ModelJournal& j, unsigned start, unsigned done) {
  const unsigned current = start + done;
  for (unsigned k = 0; k <= (unsigned)kJournalCap + 2 && k <= done; ++k) {
    // guards before and after: the call writes rects[0 .. n) and nothing else
    std::vector<JournalRect> buf(2 * kJournalCap + 2, JournalRect{-7, -7, -7, -7});
    int n = -1;
    const bool known = pp2::journal_changes_since(j, current, current - k, buf.data() + 1, &n);
    EXPECT(same(buf.front(), JournalRect{-7, -7, -7, -7}));
    EXPECT(same(buf.back(), JournalRect{-7, -7, -7, -7}));
    if (k > (unsigned)kJournalCap) {
      EXPECT(!known);
      EXPECT(n == 0);
      continue;
    }
    EXPECT(known);
    std::vector<JournalRect> want;
    for (unsigned i = done - k + 1; i <= done; ++i) {
      want.push_back(first_of(i));
      if (second_of(i).w > 0) want.push_back(second_of(i));
    }
    EXPECT(n == (int)want.size());
    for (int i = 0; i < n && i < (int)want.size(); ++i) EXPECT(same(buf[1 + i], want[i]));
    long long cells = 0;
    for (const JournalRect& r : want) cells += (long long)r.w * r.h;
    EXPECT(pp2::journal_cells(buf.data() + 1, n) == cells);
  }
}

static void run_from(unsigned start) {
  ModelJournal j;
  ask_all(j, start, 0);  // nothing recorded: only "no change" is known
  for (unsigned i = 1; i <= 3u * kJournalCap + 1; ++i) {
    j.record(start + i, first_of(i), second_of(i));
    ask_all(j, start, i);
  }
}

int main() {
  run_from(0);
  run_from(0xfffffff0u);  // the serial counter wraps inside the run

  {  // an empty journal knows nothing about a changed serial
    ModelJournal j;
    JournalRect r[2 * kJournalCap];
    int n = -1;
    EXPECT(pp2::journal_changes_since(j, 5, 5, r, &n) && n == 0);
    EXPECT(!pp2::journal_changes_since(j, 5, 4, r, &n) && n == 0);
  }
  {  // a serial ahead of the current one
    ModelJournal j;
    for (unsigned i = 1; i <= 4; ++i) j.record(i, first_of(i), second_of(i));
    JournalRect r[2 * kJournalCap];
    int n = -1;
    EXPECT(!pp2::journal_changes_since(j, 4, 5, r, &n) && n == 0);
    EXPECT(!pp2::journal_changes_since(j, 4, 9, r, &n) && n == 0);
  }
  {  // an update that was not journalled (serial 3 missing): unknown across the gap
    ModelJournal j;
    j.record(1, first_of(1), second_of(1));
    j.record(2, first_of(2), second_of(2));
    j.record(4, first_of(4), second_of(4));
    JournalRect r[2 * kJournalCap];
    int n = -1;
    EXPECT(!pp2::journal_changes_since(j, 4, 2, r, &n));
    EXPECT(!pp2::journal_changes_since(j, 4, 1, r, &n));
    EXPECT(pp2::journal_changes_since(j, 4, 3, r, &n) && n == 1 && same(r[0], first_of(4)));
  }
  {  // clear()
    ModelJournal j;
    j.record(1, first_of(1), second_of(1));
    j.clear();
    JournalRect r[2 * kJournalCap];
    int n = -1;
    EXPECT(!pp2::journal_changes_since(j, 1, 0, r, &n));
  }
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("journal capacity %d: all cases hold\n", kJournalCap);
  return 0;
}
