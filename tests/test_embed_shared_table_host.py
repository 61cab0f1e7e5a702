"""The item map of the edge embedder's row-table launch on the host (no GPU).  The launch evaluates the rows of a batch's leaders only
and learns their count on the device, so the kernel lays its items out itself with the functions of csrc/ee2_table_map.hpp; the same
functions size the grid on the host.  A host program walks the map: for every leader count 1..B and the n_rel of N = 92, 300 and a
two-chain batch, every (leader, class pair, bin tile, rel) is covered by exactly one item, no item reaches outside, and the grid the host
launches gives every live item of a one-class batch a wave of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <stdio.h>
#include <vector>
#include "ee2_table_map.hpp"
int main() {
  const int B = 45, n_rels[3] = {183, 599, 750};  // (45 samples: the most the table's byte cap admits at N = 92)
  long items = 0;
  for (int nt = 1; nt <= 2; ++nt)
    for (int r = 0; r < 3; ++r) {
      const int n_rel = n_rels[r], grid = ee2_table_max_live_blocks(B, nt, n_rel);
      for (int n_lead = 1; n_lead <= B; ++n_lead) {
        const Ee2TableMap m = ee2_table_map(n_lead, nt, n_rel);
        if (m.n_items != 4 * m.per_cc || m.rpw < 1 || m.wpg < 1 || (m.per_cc + 7) / 8 > grid) return printf("map %d %d %d\n", nt, n_rel, n_lead), 1;
        std::vector<int> seen((size_t)4 * n_lead * nt * n_rel, 0);
        for (int item = 0; item < m.n_items; ++item) {
          const Ee2TableItem it = ee2_table_item(m, item);
          if (it.cc < 0 || it.cc > 3 || it.cc != item / m.per_cc || it.lead < 0 || it.lead >= n_lead || it.jt < 0 || it.jt >= nt || it.rel0 < 0 ||
              it.rel1 > n_rel || it.rel1 - it.rel0 > m.rpw)
            return printf("item %d of %d %d %d\n", item, nt, n_rel, n_lead), 1;
          for (int rel = it.rel0; rel < it.rel1; ++rel) ++seen[(((size_t)it.cc * n_lead + it.lead) * nt + it.jt) * n_rel + rel];
          ++items;
        }
        for (size_t k = 0; k < seen.size(); ++k)
          if (seen[k] != 1) return printf("cover %zu x %d of %d %d %d\n", k, seen[k], nt, n_rel, n_lead), 1;
      }
    }
  // the flagship shape: one leader of eight samples, 599 rel, one bin tile -> one rel row per wave on 599 waves; eight leaders -> the
  // 200 ranges of three rel each per sample that the launch ran before the rows were shared
  const Ee2TableMap one = ee2_table_map(1, 1, 599), eight = ee2_table_map(8, 1, 599);
  printf("ok %ld one %d %d %d eight %d %d %d grid %d\n", items, one.wpg, one.rpw, one.per_cc, eight.wpg, eight.rpw, eight.per_cc,
         ee2_table_max_live_blocks(8, 1, 599));
  return 0;
}
"""


def test_every_row_of_every_leader_is_covered_exactly_once(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    (tmp_path / "walk.cpp").write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "framedipt_amd", "csrc"), str(tmp_path / "walk.cpp"), "-o", str(tmp_path / "walk")],
                   check=True)
    res = subprocess.run([str(tmp_path / "walk")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout
    words = res.stdout.split()
    assert words[0] == "ok" and int(words[1]) > 0
    # (wpg, rpw, per_cc) of one and of eight leaders at c4, and the grid that serves the worst count (three leaders: 3 x 599 waves)
    assert words[2:] == ["one", "599", "1", "599", "eight", "200", "3", "1600", "grid", "225"], res.stdout
