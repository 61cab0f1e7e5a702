// interface_mapped.hip — interface accuracy of a model read through a row map (include/fdipt.h, "interface accuracy through a row map";
// DESIGN.md section 7.19): fdipt_sample_interface_mapped.  Row j of everything here is a row of the REFERENCE; the model is read at
// the row the pair's map gives for it.
//
// Four launches on one stream, nothing between them on the host:
//   map kernel      a block per pair: the verdict on the pair's map (rowmap.hpp: out of range, duplicates) or on its structure
//                   indices, with n_covered and n_reference, left behind the workspace for the blocks of the other three.
//   prep kernel     a block per pair: each reference row is resolved ONCE - its model row or -1 (fd_map_row, range-checked), the
//                   atoms that take part, the RMSD atoms and its reach in both structures go to the workspace.  A row without a model
//                   row takes part under FDIPT_MAP_PENALISE with the reference's own atoms and without IF_COVERED.
//   contact kernel  interface.hip's, with the model's receptor row and ligand tile read at the resolved rows.  A residue pair is
//                   tested in the model only where both rows carry IF_COVERED; a reference-only row is pruned on the reference side
//                   alone.  Nothing is added to the tile in LDS: the resolved row is read where the tile's coordinates are loaded.
//   rmsd kernel     interface.hip's; the RMSD bits are set on covered rows only, so both superpositions run over covered rows in
//                   ascending reference rows; n_interface_covered counts the interface rows that entered irmsd.
// Under FDIPT_MAP_IGNORE IF_PRESENT and IF_COVERED coincide, and every decision and every sum is the un-mapped kernels' on the gathered
// model.
#include "interface_common.hpp"
#include "rowmap.hpp"

// the workspace: the row bits [P,N_b] u64, the reaches [P,N_b,2] f64 (both as in interface.hip), the model rows [P,N_b] i32, the verdicts [P] i32
__device__ __forceinline__ int* ifm_rows(const FdiptInterfaceArgs& a) { return (int*)((double*)a.workspace + (long)a.P * a.N * 3); }
__device__ __forceinline__ int* ifm_verdicts(const FdiptInterfaceArgs& a) { return ifm_rows(a) + (long)a.P * a.N; }

// the pair's two structures (the model has m.N_a rows, the reference a.N); false where an index is out of range
__device__ __forceinline__ bool ifm_pair(const FdiptInterfaceArgs& a, const FdiptRowMap& m, int p, IfStructure& sa, IfStructure& sb) {
  const int ia = a.pairs[2 * p], ib = a.pairs[2 * p + 1];
  if (ia < 0 || ia >= a.S || ib < 0 || ib >= a.S_b) return false;
  sa = {a.prot + (long)ia * m.N_a * a.atoms * 3, a.atom_mask_a ? a.atom_mask_a + (long)ia * m.N_a * a.atoms : nullptr, a.res_mask + (long)ia * m.N_a, a.atoms};
  sb = {a.prot_b + (long)ib * a.N * a.atoms_b * 3, a.atom_mask_b ? a.atom_mask_b + (long)ib * a.N * a.atoms_b : nullptr, a.res_mask_b + (long)ib * a.N, a.atoms_b};
  return true;
}

__global__ __launch_bounds__(FD_THREADS) void ifm_map_kernel(FdiptInterfaceArgs a, FdiptRowMap m) {
  __shared__ unsigned bits_sh[FD_MAP_WORDS];
  __shared__ int flag_sh, count_sh[2];
  const int tid = threadIdx.x, lane = tid & (FD_WAVE - 1), N = a.N, p = blockIdx.x;
  IfStructure sa, sb;
  if (!ifm_pair(a, m, p, sa, sb)) {
    if (tid == 0) ifm_verdicts(a)[p] = FDIPT_IFACE_SKIPPED, m.n_covered[p] = 0, m.n_reference[p] = 0;
    return;
  }
  const int* mp = m.map + (long)p * N;
  if (tid < 2) count_sh[tid] = 0;
  const int found = fd_map_check(mp, N, m.N_a, bits_sh, &flag_sh);  // (with barriers: count_sh is zero for everyone behind it)
  const int verdict = ((found & FDIPT_MAP_OUT_OF_RANGE) ? FDIPT_IFACE_MAP_OUT_OF_RANGE : 0) | ((found & FDIPT_MAP_DUPLICATE) ? FDIPT_IFACE_MAP_DUPLICATE : 0);
  for (int j0 = 0; j0 < N; j0 += FD_THREADS) {
    const int j = j0 + tid;
    const bool ex = j < N && sb.rm[j < N ? j : 0] != 0.f;
    const bool cov = ex && fd_map_row(mp, sa.rm, m.N_a, j) >= 0;
    const unsigned long long be = __ballot(ex), bc = __ballot(cov);
    if (lane == 0) {  // integer adds: the order changes nothing
      if (be) atomicAdd(&count_sh[1], __popcll(be));
      if (bc) atomicAdd(&count_sh[0], __popcll(bc));
    }
  }
  __syncthreads();
  if (tid == 0) {
    ifm_verdicts(a)[p] = verdict;
    m.n_covered[p] = verdict ? 0 : count_sh[0];
    m.n_reference[p] = verdict ? 0 : count_sh[1];
  }
}

__global__ __launch_bounds__(FD_THREADS) void ifm_prep_kernel(FdiptInterfaceArgs a, FdiptRowMap m, int K) {
  const int p = blockIdx.x, N = a.N, tid = threadIdx.x;
  IfStructure sa, sb;
  const bool ok = ifm_pair(a, m, p, sa, sb) && ifm_verdicts(a)[p] == 0;
  const bool penalise = m.coverage == FDIPT_MAP_PENALISE;
  const int* mp = m.map + (long)p * N;
  unsigned long long* bits = if_bits(a) + (long)p * N;
  double* reach = if_reach(a) + (long)p * N * 2;
  int* rows = ifm_rows(a) + (long)p * N;
  for (int i = tid; i < N; i += FD_THREADS) {
    for (int k = 0; k < a.I; ++k) {
      const long at = ((long)p * a.I + k) * N + i;
      a.res_native[at] = a.res_model[at] = a.res_shared[at] = a.interface_rows[at] = 0;
    }
    unsigned long long b = 0ull;
    double ra = 0.0, rb = 0.0;
    int mr = -1;
    if (ok && sb.rm[i] != 0.f) mr = fd_map_row(mp, sa.rm, m.N_a, i);
    const bool cov = mr >= 0;
    if (ok && sb.rm[i] != 0.f && (cov || penalise)) {
      b = IF_PRESENT | (cov ? IF_COVERED : 0ull);
      float caa[3] = {0.f, 0.f, 0.f}, cab[3], va[3] = {0.f, 0.f, 0.f}, vb[3];
      // an atom of a covered row takes part where both structures have it, of a reference-only row where the reference has it
      bool ca_ok = if_atom(sb, i, if_column(1, sb.atoms, 0), cab);
      if (cov) ca_ok &= if_atom(sa, mr, if_column(1, sa.atoms, 0), caa);
      if (ca_ok) b |= IF_CA_OK;
      for (int k = 0; k < K; ++k) {
        bool both = if_atom(sb, i, if_column(K, sb.atoms, k), vb);
        if (cov) both &= if_atom(sa, mr, if_column(K, sa.atoms, k), va);
        if (both) b |= 1ull << k;
      }
      if (a.mode == FDIPT_IFACE_CB) b &= (b & 2ull) ? ~1ull : ~0ull;  // CB where it takes part, else CA
      for (int k = 0; k < K; ++k) {
        if (!((b >> k) & 1ull) || !ca_ok) continue;
        if_atom(sb, i, if_column(K, sb.atoms, k), vb);
        rb = fmax(rb, if_sum_sq((double)vb[0] - (double)cab[0], (double)vb[1] - (double)cab[1], (double)vb[2] - (double)cab[2]));
        if (!cov) continue;
        if_atom(sa, mr, if_column(K, sa.atoms, k), va);
        ra = fmax(ra, if_sum_sq((double)va[0] - (double)caa[0], (double)va[1] - (double)caa[1], (double)va[2] - (double)caa[2]));
      }
      if (cov) {  // (the RMSDs compare: covered rows only)
        if (a.mode != FDIPT_IFACE_CA && sa.atoms > 1 && sb.atoms > 1) {
          for (int r = 0; r < 4; ++r)
            if (if_atom(sa, mr, if_rmsd_column(sa.atoms, r), va) & if_atom(sb, i, if_rmsd_column(sb.atoms, r), vb)) b |= 1ull << (IF_RMSD_SHIFT + r);
        } else if (ca_ok) {
          b |= 1ull << (IF_RMSD_SHIFT + 1);
        }
      }
    }
    bits[i] = b;
    reach[2 * i] = sqrt(ra);
    reach[2 * i + 1] = sqrt(rb);
    rows[i] = (b & IF_COVERED) ? mr : -1;
  }
}

template <int K, int TILE>
__global__ __launch_bounds__(FD_THREADS) void ifm_contact_kernel(FdiptInterfaceArgs a, FdiptRowMap m, int rtiles) {
  static_assert(K <= FD_WAVE && TILE % FD_WAVE == 0 && FDIPT_IFACE_ROWS <= 255 && FDIPT_IFACE_ROWS <= FD_THREADS, "a lane per atom; 8-bit counts per ligand row and tile");
  constexpr int CA = K <= 2 ? 0 : 1, SLOTS = TILE / FD_WAVE;
  constexpr unsigned long long SET = (1ull << K) - 1ull;
  __shared__ float xs[2][K * 3][TILE];  // [structure][atom, axis][ligand row of the tile]; the model's of a reference-only row are zeros
  __shared__ unsigned long long bits_sh[TILE];  // 0: no ligand row that takes part
  __shared__ double reach_sh[2][TILE];
  __shared__ unsigned lig_sh[TILE];  // native | model << 8 | shared << 16 | interface << 31 of the tile's rows
  __shared__ int cnt_sh[FDIPT_IFACE_ROWS][4];
  const int tid = threadIdx.x, lane = tid & (FD_WAVE - 1), wave = tid / FD_WAVE, N = a.N;
  const int rt = blockIdx.x % rtiles, k = (blockIdx.x / rtiles) % a.I, p = blockIdx.x / (rtiles * a.I);
  IfStructure sa, sb;
  if (!ifm_pair(a, m, p, sa, sb) || ifm_verdicts(a)[p] != 0) return;  // (the whole block; the rmsd kernel writes the pair's outputs)
  const int* side = a.sides + (long)k * N;
  const unsigned long long* wb = if_bits(a) + (long)p * N;
  const double* wr = if_reach(a) + (long)p * N * 2;
  const int* wm = ifm_rows(a) + (long)p * N;  // the model row of a row with IF_COVERED: a row of the model (the prep kernel checked it)
  const int i0 = rt * FDIPT_IFACE_ROWS;
  const bool prune = !(a.flags & FDIPT_IFACE_NO_PRUNE);
  const double cc2 = a.contact_cutoff * a.contact_cutoff, ic2 = a.interface_cutoff * a.interface_cutoff;
  const double cc_far = a.contact_cutoff * (1.0 + IF_PRUNE_MARGIN), ref_far = fmax(a.contact_cutoff, a.interface_cutoff) * (1.0 + IF_PRUNE_MARGIN);
  int mine = 0;  // tid < ROWS: row i0 + tid is a receptor row with an atom that takes part
  if (tid < FDIPT_IFACE_ROWS) {
    const int i = i0 + tid;
    mine = i < N && side[i] == FDIPT_IFACE_RECEPTOR && (wb[i] & IF_PRESENT) && (wb[i] & SET);
    cnt_sh[tid][0] = cnt_sh[tid][1] = cnt_sh[tid][2] = cnt_sh[tid][3] = 0;
  }
  if (!__syncthreads_or(mine)) return;
  for (int j0 = 0; j0 < N; j0 += TILE) {
    __syncthreads();
    int any = 0;
    for (int r = tid; r < TILE; r += FD_THREADS) {
      const int j = j0 + r;
      unsigned long long b = j < N && side[j] == FDIPT_IFACE_LIGAND ? wb[j] : 0ull;
      if (!(b & IF_PRESENT) || !(b & SET)) b = 0ull;
      bits_sh[r] = b;
      reach_sh[0][r] = b ? wr[2 * j] : 0.0;
      reach_sh[1][r] = b ? wr[2 * j + 1] : 0.0;
      lig_sh[r] = 0u;
      any |= b != 0ull;
    }
    if (!__syncthreads_or(any)) continue;  // (block-uniform) no ligand row in the tile
    for (int e = tid; e < TILE * K; e += FD_THREADS) {
      const int r = e / K, u = e % K;
      const unsigned long long b = bits_sh[r];
      float va[3] = {0.f, 0.f, 0.f}, vb[3] = {0.f, 0.f, 0.f};
      if (((b >> u) & 1ull) || (b && u == CA)) {  // (r < TILE and b != 0: j0 + r < N)
        if (b & IF_COVERED) if_atom(sa, wm[j0 + r], if_column(K, sa.atoms, u), va);
        if_atom(sb, j0 + r, if_column(K, sb.atoms, u), vb);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        xs[0][u * 3 + c][r] = va[c];
        xs[1][u * 3 + c][r] = vb[c];
      }
    }
    __syncthreads();
    unsigned lig[SLOTS], lig_if = 0u;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) lig[s] = 0u;
    for (int ii = wave; ii < FDIPT_IFACE_ROWS; ii += FD_WAVES) {
      const int i = i0 + ii;
      if (i >= N || side[i] != FDIPT_IFACE_RECEPTOR) continue;  // (wave-uniform)
      const unsigned long long bw = wb[i];
      const unsigned long long bi = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(bw >> 32)) << 32) |
                                    (unsigned)__builtin_amdgcn_readfirstlane((int)(bw & 0xffffffffull));
      if (!(bi & IF_PRESENT) || !(bi & SET)) continue;
      const bool cov_i = (bi & IF_COVERED) != 0ull;  // (wave-uniform)
      float xa[3] = {0.f, 0.f, 0.f}, xb[3] = {0.f, 0.f, 0.f};  // lane u: atom u of row i in the model and in the reference
      if (lane < K && (((bi >> lane) & 1ull) || lane == CA)) {
        if (cov_i) if_atom(sa, __builtin_amdgcn_readfirstlane(wm[i]), if_column(K, sa.atoms, lane), xa);
        if_atom(sb, i, if_column(K, sb.atoms, lane), xb);
      }
      const double ri_a = wr[2 * i], ri_b = wr[2 * i + 1];
      const double cai_a[3] = {(double)if_readlane_f(xa[0], CA), (double)if_readlane_f(xa[1], CA), (double)if_readlane_f(xa[2], CA)};
      const double cai_b[3] = {(double)if_readlane_f(xb[0], CA), (double)if_readlane_f(xb[1], CA), (double)if_readlane_f(xb[2], CA)};
      unsigned row_cnt = 0u;  // native | model << 10 | shared << 20 over this lane's ligand rows
      bool row_if = false;
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        const int jl = lane + s * FD_WAVE;
        const unsigned long long bj = bits_sh[jl];
        const bool compared = cov_i && (bj & IF_COVERED);  // the model holds both rows; else the pair is the reference's alone
        bool skip_a = !compared, skip_b = bj == 0ull;
        if (prune && bj && (bi & IF_CA_OK) && (bj & IF_CA_OK)) {
          const double db = sqrt(if_sum_sq(cai_b[0] - (double)xs[1][CA * 3][jl], cai_b[1] - (double)xs[1][CA * 3 + 1][jl], cai_b[2] - (double)xs[1][CA * 3 + 2][jl]));
          skip_b = db - ri_b - reach_sh[1][jl] > ref_far;
          if (compared) {
            const double da = sqrt(if_sum_sq(cai_a[0] - (double)xs[0][CA * 3][jl], cai_a[1] - (double)xs[0][CA * 3 + 1][jl], cai_a[2] - (double)xs[0][CA * 3 + 2][jl]));
            skip_a = da - ri_a - reach_sh[0][jl] > cc_far;
          }
        }
        const bool active = !(skip_a && skip_b);
        if (!__any(active)) continue;  // (wave-uniform)
        bool nat = false, mod = false, ifc = false;
        for (unsigned long long mi = bi & SET; mi; mi &= mi - 1ull) {  // (wave-uniform: every lane reads atom u from lane u)
          const int u = __builtin_ctzll(mi);
          const double xua = (double)if_readlane_f(xa[0], u), yua = (double)if_readlane_f(xa[1], u), zua = (double)if_readlane_f(xa[2], u);
          const double xub = (double)if_readlane_f(xb[0], u), yub = (double)if_readlane_f(xb[1], u), zub = (double)if_readlane_f(xb[2], u);
          if (!active) continue;
          for (unsigned long long mj = bj & SET; mj; mj &= mj - 1ull) {
            const int v = __builtin_ctzll(mj);
            if (!skip_b) {
              const double d2 = if_sum_sq(xub - (double)xs[1][v * 3][jl], yub - (double)xs[1][v * 3 + 1][jl], zub - (double)xs[1][v * 3 + 2][jl]);
              nat |= d2 <= cc2;
              ifc |= d2 <= ic2;
            }
            if (!skip_a) {
              const double d2 = if_sum_sq(xua - (double)xs[0][v * 3][jl], yua - (double)xs[0][v * 3 + 1][jl], zua - (double)xs[0][v * 3 + 2][jl]);
              mod |= d2 <= cc2;
            }
          }
        }
        const unsigned c = (nat ? 1u : 0u) | (mod ? 1u << 8 : 0u) | (nat && mod ? 1u << 16 : 0u);
        lig[s] += c;
        if (ifc) lig_if |= 1u << s;
        row_cnt += (nat ? 1u : 0u) + (mod ? 1u << 10 : 0u) + (nat && mod ? 1u << 20 : 0u);
        row_if |= ifc;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) row_cnt += __shfl_xor(row_cnt, o, 64);
      const bool any_if = __any(row_if);
      if (lane == 0) {
        cnt_sh[ii][0] += (int)(row_cnt & 0x3ffu);
        cnt_sh[ii][1] += (int)((row_cnt >> 10) & 0x3ffu);
        cnt_sh[ii][2] += (int)(row_cnt >> 20);
        cnt_sh[ii][3] |= any_if ? 1 : 0;
      }
    }
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const unsigned v = lig[s] | (((lig_if >> s) & 1u) << 31);
      if (lig[s]) atomicAdd(&lig_sh[lane + s * FD_WAVE], lig[s]);
      if (v >> 31) atomicOr(&lig_sh[lane + s * FD_WAVE], 1u << 31);
    }
    __syncthreads();
    for (int r = tid; r < TILE; r += FD_THREADS) {
      const unsigned v = lig_sh[r];
      if (!v) continue;  // (v != 0: bits_sh[r] != 0, so j0 + r < N)
      const long at = ((long)p * a.I + k) * N + j0 + r;
      if (v & 0xffu) atomicAdd(&a.res_native[at], (int)(v & 0xffu));
      if ((v >> 8) & 0xffu) atomicAdd(&a.res_model[at], (int)((v >> 8) & 0xffu));
      if ((v >> 16) & 0xffu) atomicAdd(&a.res_shared[at], (int)((v >> 16) & 0xffu));
      if (v >> 31) atomicOr(&a.interface_rows[at], 1);
    }
  }
  __syncthreads();
  if (mine) {  // (only this block writes the entries of its receptor rows)
    const long at = ((long)p * a.I + k) * N + i0 + tid;
    a.res_native[at] = cnt_sh[tid][0];
    a.res_model[at] = cnt_sh[tid][1];
    a.res_shared[at] = cnt_sh[tid][2];
    a.interface_rows[at] = cnt_sh[tid][3];
  }
}

// What the rmsd kernel writes for a pair that is not evaluated: the integers and fractions 0, the RMSDs and dockq NaN, the transforms 0.
__device__ __forceinline__ void if_write_skipped(const FdiptInterfaceArgs& a, long pk, int status) {
  a.n_native[pk] = a.n_model[pk] = a.n_shared[pk] = a.n_interface_rows[pk] = 0;
  a.fnat[pk] = a.fnonnat[pk] = 0.0;
  a.irmsd[pk] = a.lrmsd[pk] = a.dockq[pk] = __builtin_nan("");
  for (int c = 0; c < 9; ++c) a.interface_rotation[pk * 9 + c] = a.receptor_rotation[pk * 9 + c] = 0.0;
  for (int c = 0; c < 3; ++c) a.interface_translation[pk * 3 + c] = a.receptor_translation[pk * 3 + c] = 0.0;
  a.status[pk] = status;
}

// The outputs of one (pair, interface) from its integers (is[0 .. 2]: contacts of the reference, of the model, of both; is[3]: interface
// rows; is[4], is[5]: receptor and ligand rows that take part) and its two superpositions; one thread.
__device__ __forceinline__ void if_write_scores(const FdiptInterfaceArgs& a, long pk, const long long (&is)[6], const double (&ti)[12], const double (&tl)[12],
                                                double irmsd, double lrmsd, int st_i, int st_l) {
  int status = st_i | st_l | (is[0] == 0 ? FDIPT_IFACE_NO_NATIVE_CONTACT : 0) | (is[4] == 0 || is[5] == 0 ? FDIPT_IFACE_EMPTY_SIDE : 0);
  const double fnat = is[0] > 0 ? (double)is[2] / (double)is[0] : 0.0;
  const double fnonnat = is[1] > 0 ? (double)(is[1] - is[2]) / (double)is[1] : 0.0;
  if (is[0] == 0) irmsd = __builtin_nan("");
  const double si = irmsd / 1.5, sl = lrmsd / 8.5;
  a.n_native[pk] = (int)is[0];
  a.n_model[pk] = (int)is[1];
  a.n_shared[pk] = (int)is[2];
  a.n_interface_rows[pk] = (int)is[3];
  a.fnat[pk] = fnat;
  a.fnonnat[pk] = fnonnat;
  a.irmsd[pk] = irmsd;
  a.lrmsd[pk] = lrmsd;
  a.dockq[pk] = (fnat + 1.0 / (1.0 + si * si) + 1.0 / (1.0 + sl * sl)) / 3.0;  // (NaN where an RMSD is)
  for (int c = 0; c < 9; ++c) {
    a.interface_rotation[pk * 9 + c] = ti[c];
    a.receptor_rotation[pk * 9 + c] = tl[c];
  }
  for (int c = 0; c < 3; ++c) {
    a.interface_translation[pk * 3 + c] = ti[9 + c];
    a.receptor_translation[pk * 3 + c] = tl[9 + c];
  }
  a.status[pk] = status;
}

__global__ __launch_bounds__(FD_THREADS) void ifm_rmsd_kernel(FdiptInterfaceArgs a, FdiptRowMap m) {
  __shared__ unsigned char cls[FDIPT_IFACE_MAX_ROWS];
  __shared__ double red[FD_WAVES * 9];
  __shared__ long long red_i[FD_WAVES * 7];
  __shared__ double rot_sh[12];
  __shared__ int flag_sh;
  const int tid = threadIdx.x, N = a.N, p = blockIdx.x / a.I, k = blockIdx.x % a.I;
  const long pk = (long)p * a.I + k;
  IfStructure sa, sb;
  const bool in_range = ifm_pair(a, m, p, sa, sb);
  const int verdict = in_range ? ifm_verdicts(a)[p] : FDIPT_IFACE_SKIPPED;
  if (verdict) {
    if (tid == 0) {
      if_write_skipped(a, pk, verdict);
      a.n_interface_covered[pk] = 0;
    }
    return;
  }
  const int* side = a.sides + (long)k * N;
  const unsigned long long* wb = if_bits(a) + (long)p * N;
  const int* wm = ifm_rows(a) + (long)p * N;
  // 0 .. 2: contacts of the reference, of the model, of both; 3: interface rows; 4, 5: receptor and ligand rows that take part;
  // 6: interface rows that are covered
  long long is[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int i = tid; i < N; i += FD_THREADS) {
    const long at = pk * N + i;
    int c = 0;
    if (wb[i] & IF_PRESENT) c = side[i] == FDIPT_IFACE_RECEPTOR ? IF_CLS_RECEPTOR : side[i] == FDIPT_IFACE_LIGAND ? IF_CLS_LIGAND : 0;
    if (c && a.interface_rows[at]) c |= IF_CLS_INTERFACE;
    cls[i] = (unsigned char)c;
    if (c & IF_CLS_RECEPTOR) {
      is[0] += a.res_native[at];
      is[1] += a.res_model[at];
      is[2] += a.res_shared[at];
    }
    is[3] += (c & IF_CLS_INTERFACE) != 0;
    is[4] += (c & IF_CLS_RECEPTOR) != 0;
    is[5] += (c & IF_CLS_LIGAND) != 0;
    is[6] += (c & IF_CLS_INTERFACE) && (wb[i] & IF_COVERED);
  }
  fd_block_sum(is, red_i);  // (its barriers publish cls)
  double ti[12], tl[12], irmsd, lrmsd;
  int st_i, st_l;
  if_superpose<true>(sa, sb, wb, wm, cls, N, IF_CLS_INTERFACE, IF_CLS_INTERFACE, red, rot_sh, &flag_sh, ti, irmsd, st_i);
  if_superpose<true>(sa, sb, wb, wm, cls, N, IF_CLS_RECEPTOR, IF_CLS_LIGAND, red, rot_sh, &flag_sh, tl, lrmsd, st_l);
  if (tid != 0) return;
  const long long six[6] = {is[0], is[1], is[2], is[3], is[4], is[5]};
  if_write_scores(a, pk, six, ti, tl, irmsd, lrmsd, st_i, st_l);
  a.n_interface_covered[pk] = (int)is[6];
}

extern "C" size_t fdipt_sample_interface_mapped_workspace(int P, int N_b) {
  if (P < 1 || N_b < 1) return 0;
  return (size_t)P * N_b * (sizeof(unsigned long long) + 2 * sizeof(double) + sizeof(int)) + (size_t)P * sizeof(int);
}

extern "C" int fdipt_sample_interface_mapped(const FdiptInterfaceArgs* a, const FdiptRowMap* m, fdipt_stream_t stream) {
  if (!a || !m || a->S < 1 || a->N < 1 || a->P < 1 || a->I < 1 || a->mode < FDIPT_IFACE_CA || a->mode > FDIPT_IFACE_ALL || !(a->contact_cutoff > 0.0) ||
      !(a->interface_cutoff > 0.0) || (a->flags & ~FDIPT_IFACE_NO_PRUNE))
    return FDIPT_EINVAL;
  if (!a->prot_b || a->S_b < 1 || !a->res_mask_b || m->N_a < 1 || (m->coverage != FDIPT_MAP_IGNORE && m->coverage != FDIPT_MAP_PENALISE) || !m->map ||
      !m->n_covered || !m->n_reference || !a->n_interface_covered)
    return FDIPT_EINVAL;
  for (int atoms : {a->atoms, a->atoms_b}) {
    if (atoms != 37 && atoms != 5 && atoms != 1) return FDIPT_EINVAL;
    if ((a->mode == FDIPT_IFACE_ALL && atoms != 37) || (a->mode != FDIPT_IFACE_CA && atoms == 1)) return FDIPT_EINVAL;
  }
  if (!a->prot || !a->res_mask || !a->pairs || !a->sides || !a->n_native || !a->n_model || !a->n_shared || !a->n_interface_rows || !a->res_native ||
      !a->res_model || !a->res_shared || !a->interface_rows || !a->fnat || !a->fnonnat || !a->irmsd || !a->lrmsd || !a->dockq || !a->interface_rotation ||
      !a->interface_translation || !a->receptor_rotation || !a->receptor_translation || !a->status || !a->workspace)
    return FDIPT_EINVAL;
  if (a->N > FDIPT_IFACE_MAX_ROWS || m->N_a > FDIPT_IFACE_MAX_ROWS || a->I > FDIPT_IFACE_MAX_INTERFACES) return FDIPT_ESIZE;
  if (a->workspace_bytes < fdipt_sample_interface_mapped_workspace(a->P, a->N)) return FDIPT_ESIZE;
  const long rtiles = cdiv(a->N, FDIPT_IFACE_ROWS);
  if (rtiles * a->I * a->P > 0x7fffffffL) return FDIPT_ESIZE;
  const dim3 grid((unsigned)(rtiles * a->I * a->P)), block(FD_THREADS);
  const int K = if_set_atoms(a->mode);
  hipLaunchKernelGGL(ifm_map_kernel, dim3(a->P), block, 0, (hipStream_t)stream, *a, *m);
  FD_CHECK_LAUNCH();
  hipLaunchKernelGGL(ifm_prep_kernel, dim3(a->P), block, 0, (hipStream_t)stream, *a, *m, K);
  FD_CHECK_LAUNCH();
  if (a->mode == FDIPT_IFACE_CA)
    hipLaunchKernelGGL((ifm_contact_kernel<1, FDIPT_IFACE_TILE>), grid, block, 0, (hipStream_t)stream, *a, *m, (int)rtiles);
  else if (a->mode == FDIPT_IFACE_CB)
    hipLaunchKernelGGL((ifm_contact_kernel<2, FDIPT_IFACE_TILE>), grid, block, 0, (hipStream_t)stream, *a, *m, (int)rtiles);
  else if (a->mode == FDIPT_IFACE_BACKBONE)
    hipLaunchKernelGGL((ifm_contact_kernel<5, FDIPT_IFACE_TILE>), grid, block, 0, (hipStream_t)stream, *a, *m, (int)rtiles);
  else
    hipLaunchKernelGGL((ifm_contact_kernel<37, FDIPT_IFACE_TILE_ALL>), grid, block, 0, (hipStream_t)stream, *a, *m, (int)rtiles);
  FD_CHECK_LAUNCH();
  hipLaunchKernelGGL(ifm_rmsd_kernel, dim3(a->P * a->I), block, 0, (hipStream_t)stream, *a, *m);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
