// Stand-alone host check of pp2::masked_admit (path_planning_2d_amd/csrc/
// pp2_masked.h), the admission rule of the resident loop's masked-support
// form.  Built by tests/test_masked_admit_cpu.py with the host compiler and
// -fsanitize=address,undefined as its own executable; no GPU, no HIP.
//
// It restates the model generator per cell (base kernel, occupied neighbours
// move their mass to the centre, traps, stage cost), builds the dictionary and
// the code plane of rows [-1, rows] (zero entries for the halo rows and the
// pads) and feeds the rule made-up models: admitted ones, each rejection, and
// the off-grid cases.  Exit status 0 when every case holds.
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "pp2_masked.h"

namespace {

constexpr int kRow = 108;  // floats per dictionary row ([a][T0..T8, C] at 10 a, then L)

void base_kernel(int u, float* tp) {
  for (int i = 0; i < 9; ++i) tp[i] = 0.0f;
  static const int sup[9][4] = {{0, 1, 3, 4}, {0, 1, 2, 4}, {1, 2, 4, 5}, {0, 3, 4, 6}, {4, 4, 4, 4},
                                {2, 4, 5, 8}, {3, 4, 6, 7}, {4, 6, 7, 8}, {4, 5, 7, 8}};
  if (u == 4) {
    tp[4] = 1.0f;
    return;
  }
  for (int j = 0; j < 4; ++j) tp[sup[u][j]] = 0.1f;
  tp[u] = 0.7f;
}

struct Model {
  int H, W, wp;
  std::vector<float> cell;  // (H + 2) x wp tuples of 90 floats, row -1 first
  float* at(int y, int x) { return &cell[((size_t)(y + 1) * wp + x) * 90]; }
};

Model generate(const std::vector<uint8_t>& map, int H, int W, int wp, int gx, int gy) {
  Model m{H, W, wp, std::vector<float>((size_t)(H + 2) * wp * 90, 0.0f)};
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      uint8_t lm[9];
      for (int i = 0; i < 9; ++i) {
        const int nx = x + i % 3 - 1, ny = y + i / 3 - 1;
        lm[i] = (nx < 0 || nx >= W || ny < 0 || ny >= H) ? 1 : map[(size_t)ny * W + nx];
      }
      float* d = m.at(y, x);
      for (int u = 0; u < 9; ++u) {
        float tp[9], nm[9];
        base_kernel(u, tp);
        for (int i = 0; i < 9; ++i) nm[i] = lm[4] == 1 ? (i == 4 ? 1.0f : 0.0f) : tp[i];
        for (int i = 0; i < 9; ++i)
          if (lm[i] == 1 && i != 4) {
            tp[4] += tp[i];
            tp[i] = 0.0f;
          }
        if (lm[4] == 1) {
          for (int i = 0; i < 9; ++i) tp[i] = 0.0f;
          tp[4] = 1.0f;
        }
        float c = 0.0f;
        for (int i = 0; i < 9; ++i) c = __builtin_fmaf(lm[i] == 1 ? 2.0f : 1.0f, nm[i], c);
        if (u == 4) c = (x == gx && y == gy) ? 0.0f : 2.0f;
        for (int i = 0; i < 9; ++i) d[u * 10 + i] = tp[i];
        d[u * 10 + 9] = c;
      }
    }
  return m;
}

struct Coded {
  std::vector<uint16_t> code;
  std::vector<float> dict;
  int E = 0;
};

Coded encode(Model& m) {
  Coded c;
  std::map<std::vector<uint32_t>, int> ids;
  c.code.resize((size_t)(m.H + 2) * m.wp);
  for (size_t i = 0; i < c.code.size(); ++i) {
    std::vector<uint32_t> key(90);
    std::memcpy(key.data(), &m.cell[i * 90], 360);
    auto it = ids.find(key);
    if (it == ids.end()) {
      it = ids.emplace(key, c.E++).first;
      c.dict.resize((size_t)c.E * kRow, 0.0f);
      std::memcpy(&c.dict[(size_t)(c.E - 1) * kRow], &m.cell[i * 90], 360);
    }
    c.code[i] = (uint16_t)it->second;
  }
  return c;
}

pp2::MaskedModel admit(Model& m, Coded* out = nullptr) {
  Coded c = encode(m);
  pp2::MaskedModel r =
      pp2::masked_admit(c.code.data(), m.wp, m.H, c.dict.data(), c.E, kRow, 0.95f);
  if (out) *out = c;
  return r;
}

std::vector<uint8_t> scatter_map(int H, int W, unsigned seed, int percent) {
  std::vector<uint8_t> map((size_t)H * W, 0);
  unsigned s = seed;
  for (auto& v : map) {
    s = s * 1664525u + 1013904223u;
    v = (s >> 16) % 100 < (unsigned)percent;
  }
  return map;
}

int fails = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAIL: %s\n", what);
    ++fails;
  }
}

}  // namespace

int main() {
  const int H = 9, W = 13, wp = 16;
  std::vector<uint8_t> map = scatter_map(H, W, 7u, 25);
  // the fixed cells of the cases below
  auto set = [&](int y, int x, int v) { map[(size_t)y * W + x] = (uint8_t)v; };
  const int gy = 4, gx = 6;
  set(gy, gx, 0);
  for (int dy = -1; dy <= 1; ++dy)  // a walled-in free cell at (2, 3)
    for (int dx = -1; dx <= 1; ++dx) set(2 + dy, 3 + dx, dy || dx);
  set(0, 0, 0);  // a free corner cell with its in-grid neighbours occupied
  set(0, 1, 1); set(1, 0, 1); set(1, 1, 1);
  set(8, 9, 0);  // a free cell on the bottom edge, likewise
  set(8, 8, 1); set(8, 10, 1); set(7, 8, 1); set(7, 9, 1); set(7, 10, 1);
  set(5, 12, 0);  // a free cell at x = W - 1 with free neighbours (pads beside it)
  set(4, 12, 0); set(6, 12, 0); set(5, 11, 0);
  set(gy, gx + 1, 1);  // the goal next to an occupied cell

  {  // the generated model: admitted, the generator's weights, F as the map says
    Model m = generate(map, H, W, wp, gx, gy);
    Coded c;
    const pp2::MaskedModel r = admit(m, &c);
    expect(r.ok, "generated model admitted");
    expect(r.w_main == 0.7f && r.w_side == 0.1f, "weights 0.7 / 0.1");
    bool f_ok = r.ok;
    for (int y = -1; y <= H && f_ok; ++y)
      for (int x = 0; x < wp; ++x) {
        const bool in = y >= 0 && y < H && x < W;
        const bool want = !in || map[(size_t)y * W + x] == 1;
        if ((r.blocked[c.code[(size_t)(y + 1) * wp + x]] != 0) != want) f_ok = false;
      }
    expect(f_ok, "F == occupied or off the grid (the walled-in and edge cells are free)");
  }
  {  // no occupied cell at all
    std::vector<uint8_t> open((size_t)H * W, 0);
    Model m = generate(open, H, W, wp, gx, gy);
    const pp2::MaskedModel r = admit(m);
    expect(r.ok && r.w_main == 0.7f && r.w_side == 0.1f, "open map admitted");
  }
  {  // every cell occupied: nothing holds a weight
    std::vector<uint8_t> full((size_t)H * W, 1);
    Model m = generate(full, H, W, wp, -1, -1);
    const pp2::MaskedModel r = admit(m);
    expect(r.ok && r.w_main == 0.0f && r.w_side == 0.0f, "full map admitted, weights +0");
  }
  {  // one cell's off-centre weight changed
    Model m = generate(map, H, W, wp, gx, gy);
    float* d = m.at(5, 11);  // action 2's side weight towards the free cell (5, 12)
    expect(d[2 * 10 + 5] == 0.1f, "(the cell holds the side weight)");
    d[2 * 10 + 5] = 0.125f;
    expect(!admit(m).ok, "one off-centre weight changed: rejected");
  }
  {  // a weight set to +0 although the neighbour is free
    Model m = generate(map, H, W, wp, gx, gy);
    m.at(5, 11)[5 * 10 + 5] = 0.0f;
    expect(!admit(m).ok, "a zero weight towards a free cell: rejected");
  }
  {  // a blocked cell whose cost differs for one action
    Model m = generate(map, H, W, wp, gx, gy);
    expect(map[(size_t)2 * W + 2] == 1, "(an occupied cell)");
    m.at(2, 2)[7 * 10 + 9] = 3.0f;
    expect(!admit(m).ok, "a blocked cell's cost differs by action: rejected");
  }
  {  // one action's side weight changed everywhere
    Model m = generate(map, H, W, wp, gx, gy);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        float* d = m.at(y, x);
        for (int i = 0; i < 9; ++i)
          if (i != 4 && d[5 * 10 + i] == 0.1f) d[5 * 10 + i] = 0.05f;
      }
    expect(!admit(m).ok, "one action's side weight changed everywhere: rejected");
  }
  {  // the goal on an occupied cell: its costs differ, its neighbours' weights are +0
    Model m = generate(map, H, W, wp, gx + 1, gy);
    expect(!admit(m).ok, "goal on an occupied cell: rejected");
  }
  {  // off the grid counts as blocked: a weight that points off the grid
    Model m = generate(map, H, W, wp, gx, gy);
    expect(m.at(0, 0)[1 * 10 + 1] == 0.0f, "(action 1 at row 0 points at the halo row)");
    m.at(0, 0)[1 * 10 + 1] = 0.7f;
    expect(!admit(m).ok, "a weight towards the halo row: rejected");
  }
  {  // ... and one that points at a pad column
    Model m = generate(map, H, W, wp, gx, gy);
    expect(m.at(5, 12)[5 * 10 + 5] == 0.0f, "(action 5 at x = W - 1 points at a pad)");
    m.at(5, 12)[5 * 10 + 5] = 0.7f;
    expect(!admit(m).ok, "a weight towards a pad column: rejected");
  }
  {  // a grid as wide as its row stride: x = -1 and x = wp are off the plane
    const int W2 = 16;
    std::vector<uint8_t> mp = scatter_map(H, W2, 11u, 20);
    mp[(size_t)3 * W2] = 0;
    mp[(size_t)3 * W2 + W2 - 1] = 0;
    mp[(size_t)5 * W2 + 5] = 0;
    Model m = generate(mp, H, W2, W2, 5, 5);
    expect(admit(m).ok, "width == row stride admitted");
    m.at(3, 0)[3 * 10 + 3] = 0.7f;  // towards x = -1
    expect(!admit(m).ok, "a weight towards x = -1: rejected");
  }
  {  // a code outside the dictionary
    Model m = generate(map, H, W, wp, gx, gy);
    Coded c = encode(m);
    c.code[17] = (uint16_t)c.E;
    expect(!pp2::masked_admit(c.code.data(), wp, H, c.dict.data(), c.E, kRow, 0.95f).ok,
           "a code outside the dictionary: rejected");
    expect(!pp2::masked_admit(c.code.data(), wp, H, c.dict.data(), 0, kRow, 0.95f).ok,
           "an empty dictionary: rejected");
  }
  if (fails == 0) std::printf("masked_admit: all cases hold\n");
  return fails == 0 ? 0 : 1;
}
