// Stand-alone driver of the grouped weight-gradient plan (csrc/mv_gemm_group.h): the table builder, the tail rule and the
// unit -> (problem, tile, K-slice) map over the cases of tests/test_gemm_grouped_cpu.py, for the host sanitizers:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined tests/native/group_plan_check.cpp -o group_plan_check
//   ./group_plan_check          (prints "ok" and exits 0; any mismatch or sanitizer report is a failure)
// Plain C++: it also builds with `c++ -std=c++17 -fsanitize=address,undefined`.  Pointers are fake and never dereferenced.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <tuple>
#include <vector>
#include "../../multi-modality-self-supervision_amd/csrc/mv_gemm_group.h"

struct Shape { int No, Ko, rows; };
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

static std::vector<mv_group_problem> problems(const std::vector<Shape>& s) {
  std::vector<mv_group_problem> p;
  for (size_t i = 0; i < s.size(); ++i) {
    const uintptr_t base = 0x10000 + 0x100000 * (3 * i);
    p.push_back({(const void*)base, (const void*)(base + 0x100000), (void*)(base + 0x200000), (s[i].No + 7) / 8 * 8, (s[i].Ko + 7) / 8 * 8, s[i].Ko,
                 s[i].No, s[i].Ko, s[i].rows});
  }
  return p;
}

// every tile exactly once over its whole contraction; returns the header
static MvGroupHeader check_plan(const std::vector<Shape>& s, int G) {
  const std::vector<mv_group_problem> p = problems(s);
  std::vector<char> table(mv_group_table_bytes((int)p.size()));
  REQUIRE(mv_group_fill(MV_BF16, (int)p.size(), p.data(), G, table.data(), table.size()) == MV_OK);
  REQUIRE(mv_group_check_table(MV_BF16, (int)p.size(), table.data()) == MV_OK);
  const MvGroupHeader h = *(const MvGroupHeader*)table.data();
  const MvGroupEntry* e = (const MvGroupEntry*)(table.data() + sizeof(MvGroupHeader));
  std::map<std::tuple<int, int, int>, std::vector<MvGroupUnit>> seen;
  for (int u = 0; u < h.direct + h.tail * h.split; ++u) {
    const MvGroupUnit d = mv_group_decode(h, e, u);
    REQUIRE(d.problem >= 0 && d.problem < h.count && d.m0 >= 0 && d.m0 < s[d.problem].No && d.n0 >= 0 && d.n0 < s[d.problem].Ko);
    seen[{d.problem, d.m0, d.n0}].push_back(d);
  }
  REQUIRE((int)seen.size() == h.units);
  std::set<int> flat;
  for (auto& kv : seen) {
    const int rows = s[std::get<0>(kv.first)].rows;
    flat.insert(kv.second[0].tile);
    if (kv.second[0].tile < h.direct) {
      REQUIRE(kv.second.size() == 1 && kv.second[0].slice == -1 && kv.second[0].kbeg == 0 && kv.second[0].kend == rows);
    } else {
      REQUIRE((int)kv.second.size() == h.split);
      std::vector<int> covered(rows, 0);
      for (const MvGroupUnit& d : kv.second)
        for (int k = d.kbeg; k < d.kend; ++k) ++covered[k];
      for (int c : covered) REQUIRE(c == 1);
    }
  }
  REQUIRE((int)flat.size() == h.units && *flat.begin() == 0 && *flat.rbegin() == h.units - 1);
  REQUIRE(mv_group_workspace_bytes(table.data()) == (h.split > 1 ? (size_t)h.tail * h.split * 65536 * 4 : 0));
  return h;
}

int main() {
  const int G = 256;
  for (int U : {1, G - 1, G, G + 1}) {
    const std::vector<Shape> s = U == 1 ? std::vector<Shape>{{256, 200, 4100}} : std::vector<Shape>{{256 * (U - 1), 256, 4100}, {130, 70, 333}};
    const MvGroupHeader h = check_plan(s, G);
    REQUIRE(h.direct == U && h.tail == 0 && h.split == 1);
  }
  std::vector<Shape> layers;
  for (int l = 0; l < 11; ++l)
    for (Shape q : {Shape{768, 3072, 25483}, Shape{3072, 768, 25483}, Shape{768, 768, 25483}, Shape{2304, 768, 25483}}) layers.push_back(q);
  MvGroupHeader h = check_plan(layers, G);
  REQUIRE(h.units == 1188 && h.direct == 1024 && h.tail == 164 && h.split == 3);
  const int tail_cases[][3] = {{100, 256, 2}, {180, 256, 1}, {164, 256, 3}, {1, 3, 3}, {2, 5, 2}, {3, 4, 1}, {0, 7, 1}, {40, 256, 5}, {10, 256, 1}};
  for (auto& c : tail_cases) {
    REQUIRE(mv_group_tail_split(c[0], c[1]) == c[2]);
    h = check_plan({{256 * (c[1] + c[0]), 256, 2048}}, c[1]);
    REQUIRE(h.split == c[2] && h.tail == (c[2] > 1 ? c[0] : 0));
  }
  h = check_plan({{256 * 7, 256, 640}, {128, 64, 100}}, 7);          // empty slices of a short contraction
  REQUIRE(h.direct == 7 && h.tail == 1 && h.split == 5);
  h = check_plan({{256, 256, 320}, {512, 256, 448}, {768, 256, 448}, {200, 136, 333}}, 3);
  REQUIRE(h.direct == 6 && h.tail == 1 && h.split == 3);
  // rejects: nothing is written
  std::vector<char> table(mv_group_table_bytes(1), 0);
  std::vector<mv_group_problem> p = problems({{768, 768, 1 << 21}});
  REQUIRE(mv_group_fill(MV_BF16, 1, p.data(), G, table.data(), table.size()) == MV_E_SHAPE);       // an operand over 2 GiB
  p = problems({{768, 768, 4096}});
  p[0].A = (const void*)0x10008;
  REQUIRE(mv_group_fill(MV_BF16, 1, p.data(), G, table.data(), table.size()) == MV_E_SHAPE);
  REQUIRE(mv_group_fill(MV_F32, 1, p.data(), G, table.data(), table.size()) == MV_E_DTYPE);
  REQUIRE(mv_group_fill(MV_BF16, 0, p.data(), G, table.data(), table.size()) == MV_E_ARG);
  REQUIRE(mv_group_fill(MV_BF16, 1, nullptr, G, table.data(), table.size()) == MV_E_ARG);
  REQUIRE(mv_group_check_table(MV_BF16, 1, table.data()) == MV_E_ARG && mv_group_check_table(MV_BF16, 1, nullptr) == MV_E_ARG);
  for (char c : table) REQUIRE(c == 0);
  std::puts("ok");
  return 0;
}
