// interface.hip — interface accuracy of complexes on the device (include/fdipt.h, "interface accuracy"): the
// contacts across an interface in the reference and in the model, fnat, fnonnat, interface RMSD, ligand RMSD and DockQ of P pairs
// (model a, reference b) in row correspondence on I interfaces, all in float64.
//
// Three launches on one stream, nothing between them on the host:
//   prep kernel     a block per pair: per row the atoms of the set that take part (they exist in both structures), the RMSD atoms, and
//                   the row's reach in both structures (largest CA-to-atom distance) go to the workspace; the per-row outputs of the
//                   pair are zeroed.
//   contact kernel  a block per (pair, interface, tile of FDIPT_IFACE_ROWS rows).  The ligand rows pass through LDS in tiles of TILE rows
//                   (256 at <= 5 atoms per row, 64 at 37: a block's LDS stays below 64 KB); a tile without a ligand row is skipped before
//                   a coordinate is read.  A wave serves the block's receptor rows wave, wave + 4, ...: lane u holds atom u of the row in
//                   both structures (the loop over u reads it with v_readlane), lane l takes the ligand rows l, l + 64, ... of the tile.
//                   One residue pair yields its three bits together: contact of the reference, contact of the model, interface.  A
//                   receptor row's counts belong to its block (plain stores); a ligand row's are summed in LDS per tile and flushed with
//                   integer atomics.
//   rmsd kernel     a block per (pair, interface): the integers of the pair (the receptor rows' counts summed), then two superpositions
//                   as evaluate.hip forms them (centroids, covariance, fd_horn_rotation on one thread, deviations; fd_block_sum's order).
// Integers only leave the contact kernel, so no order of anything changes a bit of them; pruning skips a residue pair of a structure
// only where the triangle inequality proves that no atom pair of it can be within the cutoff.
#include "interface_common.hpp"

// the pair's two structures; false where an index is out of range
__device__ __forceinline__ bool if_pair(const FdiptInterfaceArgs& a, int p, IfStructure& sa, IfStructure& sb) {
  const int ia = a.pairs[2 * p], ib = a.pairs[2 * p + 1], s_b = a.prot_b ? a.S_b : a.S;
  if (ia < 0 || ia >= a.S || ib < 0 || ib >= s_b) return false;
  const int atoms_b = a.prot_b ? a.atoms_b : a.atoms;
  sa = {a.prot + (long)ia * a.N * a.atoms * 3, a.atom_mask_a ? a.atom_mask_a + (long)ia * a.N * a.atoms : nullptr, a.res_mask + (long)ia * a.N, a.atoms};
  sb = {(a.prot_b ? a.prot_b : a.prot) + (long)ib * a.N * atoms_b * 3, a.atom_mask_b ? a.atom_mask_b + (long)ib * a.N * atoms_b : nullptr,
        (a.prot_b ? a.res_mask_b : a.res_mask) + (long)ib * a.N, atoms_b};
  return true;
}

__global__ __launch_bounds__(FD_THREADS) void iface_prep_kernel(FdiptInterfaceArgs a, int K) {
  const int p = blockIdx.x, N = a.N, tid = threadIdx.x;
  IfStructure sa, sb;
  const bool ok = if_pair(a, p, sa, sb);
  unsigned long long* bits = if_bits(a) + (long)p * N;
  double* reach = if_reach(a) + (long)p * N * 2;
  for (int i = tid; i < N; i += FD_THREADS) {
    for (int k = 0; k < a.I; ++k) {
      const long at = ((long)p * a.I + k) * N + i;
      a.res_native[at] = a.res_model[at] = a.res_shared[at] = a.interface_rows[at] = 0;
    }
    unsigned long long b = 0ull;
    double ra = 0.0, rb = 0.0;
    if (ok && sa.rm[i] != 0.f && sb.rm[i] != 0.f) {
      b = IF_PRESENT;
      float caa[3], cab[3], va[3], vb[3];
      const bool ca_ok = if_atom(sa, i, if_column(1, sa.atoms, 0), caa) & if_atom(sb, i, if_column(1, sb.atoms, 0), cab);
      if (ca_ok) b |= IF_CA_OK;
      for (int k = 0; k < K; ++k)
        if (if_atom(sa, i, if_column(K, sa.atoms, k), va) & if_atom(sb, i, if_column(K, sb.atoms, k), vb)) b |= 1ull << k;
      if (a.mode == FDIPT_IFACE_CB) b &= (b & 2ull) ? ~1ull : ~0ull;  // CB where both structures have it, else CA
      for (int k = 0; k < K; ++k) {
        if (!((b >> k) & 1ull) || !ca_ok) continue;
        if_atom(sa, i, if_column(K, sa.atoms, k), va);
        if_atom(sb, i, if_column(K, sb.atoms, k), vb);
        ra = fmax(ra, if_sum_sq((double)va[0] - (double)caa[0], (double)va[1] - (double)caa[1], (double)va[2] - (double)caa[2]));
        rb = fmax(rb, if_sum_sq((double)vb[0] - (double)cab[0], (double)vb[1] - (double)cab[1], (double)vb[2] - (double)cab[2]));
      }
      if (a.mode != FDIPT_IFACE_CA && sa.atoms > 1 && sb.atoms > 1) {
        for (int r = 0; r < 4; ++r)
          if (if_atom(sa, i, if_rmsd_column(sa.atoms, r), va) & if_atom(sb, i, if_rmsd_column(sb.atoms, r), vb)) b |= 1ull << (IF_RMSD_SHIFT + r);
      } else if (ca_ok) {
        b |= 1ull << (IF_RMSD_SHIFT + 1);
      }
    }
    bits[i] = b;
    reach[2 * i] = sqrt(ra);
    reach[2 * i + 1] = sqrt(rb);
  }
}

template <int K, int TILE>
__global__ __launch_bounds__(FD_THREADS) void iface_contact_kernel(FdiptInterfaceArgs a, int rtiles) {
  static_assert(K <= FD_WAVE && TILE % FD_WAVE == 0 && FDIPT_IFACE_ROWS <= 255 && FDIPT_IFACE_ROWS <= FD_THREADS, "a lane per atom; 8-bit counts per ligand row and tile");
  constexpr int CA = K <= 2 ? 0 : 1, SLOTS = TILE / FD_WAVE;
  constexpr unsigned long long SET = (1ull << K) - 1ull;
  __shared__ float xs[2][K * 3][TILE];  // [structure][atom, axis][ligand row of the tile]
  __shared__ unsigned long long bits_sh[TILE];  // 0: no ligand row that takes part
  __shared__ double reach_sh[2][TILE];
  __shared__ unsigned lig_sh[TILE];  // native | model << 8 | shared << 16 | interface << 31 of the tile's rows
  __shared__ int cnt_sh[FDIPT_IFACE_ROWS][4];
  const int tid = threadIdx.x, lane = tid & (FD_WAVE - 1), wave = tid / FD_WAVE, N = a.N;
  const int rt = blockIdx.x % rtiles, k = (blockIdx.x / rtiles) % a.I, p = blockIdx.x / (rtiles * a.I);
  IfStructure sa, sb;
  if (!if_pair(a, p, sa, sb)) return;  // (the whole block; the rmsd kernel writes the pair's outputs)
  const int* side = a.sides + (long)k * N;
  const unsigned long long* wb = if_bits(a) + (long)p * N;
  const double* wr = if_reach(a) + (long)p * N * 2;
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
        if_atom(sa, j0 + r, if_column(K, sa.atoms, u), va);
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
    for (int m = 0; m < SLOTS; ++m) lig[m] = 0u;
    for (int ii = wave; ii < FDIPT_IFACE_ROWS; ii += FD_WAVES) {
      const int i = i0 + ii;
      if (i >= N || side[i] != FDIPT_IFACE_RECEPTOR) continue;  // (wave-uniform)
      const unsigned long long bw = wb[i];
      const unsigned long long bi = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(bw >> 32)) << 32) |
                                    (unsigned)__builtin_amdgcn_readfirstlane((int)(bw & 0xffffffffull));
      if (!(bi & IF_PRESENT) || !(bi & SET)) continue;
      float xa[3] = {0.f, 0.f, 0.f}, xb[3] = {0.f, 0.f, 0.f};  // lane u: atom u of row i in the model and in the reference
      if (lane < K && (((bi >> lane) & 1ull) || lane == CA)) {
        if_atom(sa, i, if_column(K, sa.atoms, lane), xa);
        if_atom(sb, i, if_column(K, sb.atoms, lane), xb);
      }
      const double ri_a = wr[2 * i], ri_b = wr[2 * i + 1];
      const double cai_a[3] = {(double)if_readlane_f(xa[0], CA), (double)if_readlane_f(xa[1], CA), (double)if_readlane_f(xa[2], CA)};
      const double cai_b[3] = {(double)if_readlane_f(xb[0], CA), (double)if_readlane_f(xb[1], CA), (double)if_readlane_f(xb[2], CA)};
      unsigned row_cnt = 0u;  // native | model << 10 | shared << 20 over this lane's ligand rows
      bool row_if = false;
#pragma unroll
      for (int m = 0; m < SLOTS; ++m) {
        const int jl = lane + m * FD_WAVE;
        const unsigned long long bj = bits_sh[jl];
        bool skip_a = bj == 0ull, skip_b = bj == 0ull;
        if (prune && bj && (bi & IF_CA_OK) && (bj & IF_CA_OK)) {
          const double da = sqrt(if_sum_sq(cai_a[0] - (double)xs[0][CA * 3][jl], cai_a[1] - (double)xs[0][CA * 3 + 1][jl], cai_a[2] - (double)xs[0][CA * 3 + 2][jl]));
          const double db = sqrt(if_sum_sq(cai_b[0] - (double)xs[1][CA * 3][jl], cai_b[1] - (double)xs[1][CA * 3 + 1][jl], cai_b[2] - (double)xs[1][CA * 3 + 2][jl]));
          skip_a = da - ri_a - reach_sh[0][jl] > cc_far;
          skip_b = db - ri_b - reach_sh[1][jl] > ref_far;
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
        lig[m] += c;
        if (ifc) lig_if |= 1u << m;
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
    for (int m = 0; m < SLOTS; ++m) {
      const unsigned v = lig[m] | (((lig_if >> m) & 1u) << 31);
      if (lig[m]) atomicAdd(&lig_sh[lane + m * FD_WAVE], lig[m]);
      if (v >> 31) atomicOr(&lig_sh[lane + m * FD_WAVE], 1u << 31);
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

__global__ __launch_bounds__(FD_THREADS) void iface_rmsd_kernel(FdiptInterfaceArgs a) {
  __shared__ unsigned char cls[FDIPT_IFACE_MAX_ROWS];
  __shared__ double red[FD_WAVES * 9];
  __shared__ long long red_i[FD_WAVES * 6];
  __shared__ double rot_sh[12];
  __shared__ int flag_sh;
  const int tid = threadIdx.x, N = a.N, p = blockIdx.x / a.I, k = blockIdx.x % a.I;
  const long pk = (long)p * a.I + k;
  IfStructure sa, sb;
  if (!if_pair(a, p, sa, sb)) {
    if (tid == 0) {
      a.n_native[pk] = a.n_model[pk] = a.n_shared[pk] = a.n_interface_rows[pk] = 0;
      a.fnat[pk] = a.fnonnat[pk] = 0.0;
      a.irmsd[pk] = a.lrmsd[pk] = a.dockq[pk] = __builtin_nan("");
      for (int c = 0; c < 9; ++c) a.interface_rotation[pk * 9 + c] = a.receptor_rotation[pk * 9 + c] = 0.0;
      for (int c = 0; c < 3; ++c) a.interface_translation[pk * 3 + c] = a.receptor_translation[pk * 3 + c] = 0.0;
      a.status[pk] = FDIPT_IFACE_SKIPPED;
    }
    return;
  }
  const int* side = a.sides + (long)k * N;
  const unsigned long long* wb = if_bits(a) + (long)p * N;
  // 0 .. 2: contacts of the reference, of the model, of both; 3: interface rows; 4, 5: receptor and ligand rows that take part
  long long is[6] = {0, 0, 0, 0, 0, 0};
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
  }
  fd_block_sum(is, red_i);  // (its barriers publish cls)
  double ti[12], tl[12], irmsd, lrmsd;
  int st_i, st_l;
  if_superpose<false>(sa, sb, wb, nullptr, cls, N, IF_CLS_INTERFACE, IF_CLS_INTERFACE, red, rot_sh, &flag_sh, ti, irmsd, st_i);
  if_superpose<false>(sa, sb, wb, nullptr, cls, N, IF_CLS_RECEPTOR, IF_CLS_LIGAND, red, rot_sh, &flag_sh, tl, lrmsd, st_l);
  if (tid != 0) return;
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

extern "C" size_t fdipt_sample_interface_workspace(int P, int N) {
  if (P < 1 || N < 1) return 0;
  return (size_t)P * N * (sizeof(unsigned long long) + 2 * sizeof(double));
}

extern "C" int fdipt_sample_interface(const FdiptInterfaceArgs* a, fdipt_stream_t stream) {
  if (!a || a->S < 1 || a->N < 1 || a->P < 1 || a->I < 1 || a->mode < FDIPT_IFACE_CA || a->mode > FDIPT_IFACE_ALL || !(a->contact_cutoff > 0.0) ||
      !(a->interface_cutoff > 0.0) || (a->flags & ~FDIPT_IFACE_NO_PRUNE))
    return FDIPT_EINVAL;
  const int atoms_b = a->prot_b ? a->atoms_b : a->atoms;
  for (int atoms : {a->atoms, atoms_b}) {
    if (atoms != 37 && atoms != 5 && atoms != 1) return FDIPT_EINVAL;
    if ((a->mode == FDIPT_IFACE_ALL && atoms != 37) || (a->mode != FDIPT_IFACE_CA && atoms == 1)) return FDIPT_EINVAL;
  }
  if (a->prot_b && (a->S_b < 1 || !a->res_mask_b)) return FDIPT_EINVAL;
  if (!a->prot || !a->res_mask || !a->pairs || !a->sides || !a->n_native || !a->n_model || !a->n_shared || !a->n_interface_rows || !a->res_native ||
      !a->res_model || !a->res_shared || !a->interface_rows || !a->fnat || !a->fnonnat || !a->irmsd || !a->lrmsd || !a->dockq || !a->interface_rotation ||
      !a->interface_translation || !a->receptor_rotation || !a->receptor_translation || !a->status || !a->workspace)
    return FDIPT_EINVAL;
  if (a->N > FDIPT_IFACE_MAX_ROWS || a->I > FDIPT_IFACE_MAX_INTERFACES) return FDIPT_ESIZE;
  if (a->workspace_bytes < fdipt_sample_interface_workspace(a->P, a->N)) return FDIPT_ESIZE;
  const long rtiles = cdiv(a->N, FDIPT_IFACE_ROWS);
  if (rtiles * a->I * a->P > 0x7fffffffL) return FDIPT_ESIZE;
  const dim3 grid((unsigned)(rtiles * a->I * a->P)), block(FD_THREADS);
  const int K = if_set_atoms(a->mode);
  hipLaunchKernelGGL(iface_prep_kernel, dim3(a->P), block, 0, (hipStream_t)stream, *a, K);
  FD_CHECK_LAUNCH();
  if (a->mode == FDIPT_IFACE_CA)
    hipLaunchKernelGGL((iface_contact_kernel<1, FDIPT_IFACE_TILE>), grid, block, 0, (hipStream_t)stream, *a, (int)rtiles);
  else if (a->mode == FDIPT_IFACE_CB)
    hipLaunchKernelGGL((iface_contact_kernel<2, FDIPT_IFACE_TILE>), grid, block, 0, (hipStream_t)stream, *a, (int)rtiles);
  else if (a->mode == FDIPT_IFACE_BACKBONE)
    hipLaunchKernelGGL((iface_contact_kernel<5, FDIPT_IFACE_TILE>), grid, block, 0, (hipStream_t)stream, *a, (int)rtiles);
  else
    hipLaunchKernelGGL((iface_contact_kernel<37, FDIPT_IFACE_TILE_ALL>), grid, block, 0, (hipStream_t)stream, *a, (int)rtiles);
  FD_CHECK_LAUNCH();
  hipLaunchKernelGGL(iface_rmsd_kernel, dim3(a->P * a->I), block, 0, (hipStream_t)stream, *a);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
