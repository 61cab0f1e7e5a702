// ee2_table_map.hpp — work items of the edge embedder's row-table launch (edge_embed2.hip: edge_embed2_kernel<..., TABLE>).
//
// The launch evaluates the rows of the LEADERS of a batch only (samples whose layer-1 rows no earlier sample already provides), and
// only the device knows how many leaders a batch has.  The kernel therefore derives its items from the leader count with the functions
// below; the host uses the same functions to size the grid for the worst leader count.  Plain C++ (no HIP), so that a host program can
// walk the map (tests/test_embed_shared_table_host.py).
#pragma once
#if defined(__HIPCC__)
#define EE2_HD __host__ __device__ __forceinline__
#else
#define EE2_HD inline
#endif

#define EE2_TABLE_WAVES 2048  // waves of one round of the persistent launch (256 blocks of 8)

// one item = (class pair cc, leader k of n_lead, bin tile jt of nt, rel range [rel0, rel1)); items are class-pair major, so that the live
// items of a one-class batch (de novo sampling) are the first per_cc ones
struct Ee2TableMap {
  int nt, n_rel, wpg, rpw, per_cc, n_items;
};
struct Ee2TableItem {
  int cc, lead, jt, rel0, rel1;
};
EE2_HD Ee2TableMap ee2_table_map(int n_lead, int nt, int n_rel) {
  Ee2TableMap m;
  m.nt = nt;
  m.n_rel = n_rel;
  const int n_groups = n_lead * nt;
  int wpg = EE2_TABLE_WAVES / n_groups < 1 ? 1 : EE2_TABLE_WAVES / n_groups;  // ranges per group so that the live items fill one round
  if (wpg > n_rel) wpg = n_rel;
  m.rpw = (n_rel + wpg - 1) / wpg;
  m.wpg = (n_rel + m.rpw - 1) / m.rpw;
  m.per_cc = n_groups * m.wpg;
  m.n_items = 4 * m.per_cc;
  return m;
}
EE2_HD Ee2TableItem ee2_table_item(const Ee2TableMap& m, int item) {
  Ee2TableItem it;
  it.cc = item / m.per_cc;
  const int it_cc = item - it.cc * m.per_cc, grp = it_cc / m.wpg, part = it_cc - grp * m.wpg;
  it.lead = grp / m.nt;
  it.jt = grp - it.lead * m.nt;
  it.rel0 = part * m.rpw;
  it.rel1 = it.rel0 + m.rpw < m.n_rel ? it.rel0 + m.rpw : m.n_rel;
  return it;
}
// blocks of 8 waves that give every live item of a one-class batch a wave of its own, for the leader count that needs the most
EE2_HD int ee2_table_max_live_blocks(int B, int nt, int n_rel) {
  int worst = 0;
  for (int n_lead = 1; n_lead <= B; ++n_lead) {
    const int blocks = (ee2_table_map(n_lead, nt, n_rel).per_cc + 7) / 8;
    worst = blocks > worst ? blocks : worst;
  }
  return worst;
}
