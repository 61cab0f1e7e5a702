// interface_mapped.hip — interface accuracy of a model read through a row map (include/fdipt.h, "interface accuracy through a row map";
// DESIGN.md section 7.19): fdipt_sample_interface_mapped.  The prep and rmsd kernels are interface_body.hpp's in their MAPPED
// instantiations, the contact kernel is this unit's own; in front of them one small launch, a block per pair, gives the verdict on the pair's map - out of range, duplicates
// (rowmap.hpp) or a structure index out of range - with n_covered and n_reference, and leaves it behind the workspace for the blocks
// of the other three.
#include "interface_body.hpp"

__global__ __launch_bounds__(FD_THREADS) void ifm_map_kernel(FdiptInterfaceArgs a, FdiptRowMap m) {
  __shared__ FdMapLds lds;
  const int p = blockIdx.x;
  IfStructure sa, sb;
  int verdict = FDIPT_IFACE_SKIPPED, n_covered = 0, n_reference = 0;
  if (ifm_pair(a, m, p, sa, sb)) {  // (block-uniform)
    const int found = fd_map_judge(m.map + (long)p * a.N, sa.rm, sb.rm, a.N, m.N_a, lds, n_covered, n_reference);
    verdict = ((found & FDIPT_MAP_OUT_OF_RANGE) ? FDIPT_IFACE_MAP_OUT_OF_RANGE : 0) | ((found & FDIPT_MAP_DUPLICATE) ? FDIPT_IFACE_MAP_DUPLICATE : 0);
  }
  if (threadIdx.x == 0) ifm_verdicts(a)[p] = verdict, m.n_covered[p] = n_covered, m.n_reference[p] = n_reference;
}

__global__ __launch_bounds__(FD_THREADS) void ifm_prep_kernel(FdiptInterfaceArgs a, FdiptRowMap m, int K) { if_prep_body<true>(a, m, K); }

// The contact kernel is interface.hip's with the model's receptor row and ligand tile read at the resolved rows (seven lines apart):
// a residue pair is tested in the model only where both rows carry IF_COVERED, and a reference-only row is pruned on the reference
// side alone.  It stands here in full, not as an instantiation of a shared body: a change to one is a change to both.
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

__global__ __launch_bounds__(FD_THREADS) void ifm_rmsd_kernel(FdiptInterfaceArgs a, FdiptRowMap m) { if_rmsd_body<true>(a, m); }

extern "C" size_t fdipt_sample_interface_mapped_workspace(int P, int N_b) {
  if (P < 1 || N_b < 1) return 0;
  return (size_t)P * N_b * (sizeof(unsigned long long) + 2 * sizeof(double) + sizeof(int)) + (size_t)P * sizeof(int);
}

extern "C" int fdipt_sample_interface_mapped(const FdiptInterfaceArgs* a, const FdiptRowMap* m, fdipt_stream_t stream) {
  if (!m) return FDIPT_EINVAL;
  const int rc = if_check_args(a, m);
  if (rc != FDIPT_OK) return rc;
  if (a->workspace_bytes < fdipt_sample_interface_mapped_workspace(a->P, a->N)) return FDIPT_ESIZE;
  static void (*const contact[])(FdiptInterfaceArgs, FdiptRowMap, int) = {  // by FDIPT_IFACE_CA .. FDIPT_IFACE_ALL
      ifm_contact_kernel<1, FDIPT_IFACE_TILE>, ifm_contact_kernel<2, FDIPT_IFACE_TILE>, ifm_contact_kernel<5, FDIPT_IFACE_TILE>,
      ifm_contact_kernel<37, FDIPT_IFACE_TILE_ALL>};
  const int rtiles = cdiv(a->N, FDIPT_IFACE_ROWS);
  const dim3 grid((unsigned)rtiles * a->I * a->P), block(FD_THREADS);
  hipLaunchKernelGGL(ifm_map_kernel, dim3(a->P), block, 0, (hipStream_t)stream, *a, *m);
  FD_CHECK_LAUNCH();
  hipLaunchKernelGGL(ifm_prep_kernel, dim3(a->P), block, 0, (hipStream_t)stream, *a, *m, if_set_atoms(a->mode));
  FD_CHECK_LAUNCH();
  hipLaunchKernelGGL(contact[a->mode - FDIPT_IFACE_CA], grid, block, 0, (hipStream_t)stream, *a, *m, rtiles);
  FD_CHECK_LAUNCH();
  hipLaunchKernelGGL(ifm_rmsd_kernel, dim3(a->P * a->I), block, 0, (hipStream_t)stream, *a, *m);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
