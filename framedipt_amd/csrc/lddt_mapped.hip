// lddt_mapped.hip — lDDT, dRMSD and backbone FAPE of a model read through a row map (include/fdipt.h, "accuracy through a row map";
// DESIGN.md section 7.16): fdipt_sample_lddt_mapped.  The pair and reduce kernels are lddt_body.hpp's in their MAPPED instantiations;
// in front of them one small launch, a block per pair, gives the verdict on the pair's map - out of range, duplicates (rowmap.hpp) or a
// structure index out of range - with n_covered and n_reference, and leaves it behind the workspace for the blocks of the other two.
#include "lddt_body.hpp"

__global__ __launch_bounds__(FD_THREADS) void lddt_map_kernel(FdiptLddtArgs a, FdiptRowMap m) {
  __shared__ FdMapLds lds;
  const int N = a.N, p = blockIdx.x;
  const int ia = a.pairs[2 * p], ib = a.pairs[2 * p + 1];
  int verdict = FDIPT_LDDT_SKIPPED, n_covered = 0, n_reference = 0;
  if (ia >= 0 && ia < a.S && ib >= 0 && ib < a.S_b)  // (block-uniform)
    verdict = fd_map_judge(m.map + (long)p * N, a.res_mask + (long)ia * m.N_a, m.res_mask_b + (long)ib * N, N, m.N_a, lds, n_covered, n_reference);
  if (threadIdx.x == 0) ld_verdicts(a)[p] = verdict, m.n_covered[p] = n_covered, m.n_reference[p] = n_reference;
}

template <int K, int TILE>
__global__ __launch_bounds__(FD_THREADS) void lddt_pair_mapped_kernel(FdiptLddtArgs a, int tiles, FdiptRowMap m) {
  lddt_pair_body<K, TILE, true>(a, tiles, m);
}

__global__ __launch_bounds__(FD_THREADS) void lddt_reduce_mapped_kernel(FdiptLddtArgs a, int set_atoms, FdiptRowMap m) {
  lddt_reduce_body<true>(a, set_atoms, m);
}

extern "C" size_t fdipt_sample_lddt_mapped_workspace(int P, int N_b) {
  if (P < 1 || N_b < 1) return 0;
  return (size_t)P * N_b * (2 * sizeof(double) + sizeof(int)) + (size_t)P * sizeof(int);
}

extern "C" int fdipt_sample_lddt_mapped(const FdiptLddtArgs* a, const FdiptRowMap* m, fdipt_stream_t stream) {
  if (!m) return FDIPT_EINVAL;
  const int rc = ld_check_args(a, m->score_mask_b);
  if (rc != FDIPT_OK) return rc;
  if (!a->prot_b || m->N_a < 1 || (m->coverage != FDIPT_MAP_IGNORE && m->coverage != FDIPT_MAP_PENALISE) || !m->map || !m->res_mask_b || !m->n_covered ||
      !m->n_reference)
    return FDIPT_EINVAL;
  if (a->workspace_bytes < fdipt_sample_lddt_mapped_workspace(a->P, a->N)) return FDIPT_ESIZE;
  const long tiles = cdiv(a->N, FD_WAVES), K = ld_set_atoms(a->mode);
  const dim3 grid((unsigned)(tiles * a->P)), block(FD_THREADS);
  hipLaunchKernelGGL(lddt_map_kernel, dim3(a->P), block, 0, (hipStream_t)stream, *a, *m);
  FD_CHECK_LAUNCH();
  if (a->mode == FDIPT_LDDT_CA)
    hipLaunchKernelGGL((lddt_pair_mapped_kernel<1, FDIPT_LDDT_TILE>), grid, block, 0, (hipStream_t)stream, *a, (int)tiles, *m);
  else if (a->mode == FDIPT_LDDT_BACKBONE)
    hipLaunchKernelGGL((lddt_pair_mapped_kernel<4, FDIPT_LDDT_TILE>), grid, block, 0, (hipStream_t)stream, *a, (int)tiles, *m);
  else
    hipLaunchKernelGGL((lddt_pair_mapped_kernel<37, FDIPT_LDDT_TILE_ALL>), grid, block, 0, (hipStream_t)stream, *a, (int)tiles, *m);
  FD_CHECK_LAUNCH();
  hipLaunchKernelGGL(lddt_reduce_mapped_kernel, dim3(a->P), block, 0, (hipStream_t)stream, *a, (int)K, *m);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
