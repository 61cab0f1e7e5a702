// lddt.hip — superposition-free accuracy of samples on the device (include/fdipt.h, "superposition-free accuracy"): lDDT
// (openfold/utils/loss.py lddt :382, lddt_ca :438), dRMSD (compute_drmsd :1518) and backbone FAPE (compute_fape :76 as backbone_loss :152
// calls it) of P ordered pairs (model a, reference b) of structures in row correspondence, all in float64.
//
// The kernels are lddt_body.hpp's, in their instantiations without a row map.
#include "lddt_body.hpp"

template <int K, int TILE>
__global__ __launch_bounds__(FD_THREADS) void lddt_pair_kernel(FdiptLddtArgs a, int tiles) {
  lddt_pair_body<K, TILE, false>(a, tiles, FdiptRowMap{});
}

__global__ __launch_bounds__(FD_THREADS) void lddt_reduce_kernel(FdiptLddtArgs a, int set_atoms) { lddt_reduce_body<false>(a, set_atoms, FdiptRowMap{}); }

extern "C" size_t fdipt_sample_lddt_workspace(int P, int N) {
  if (P < 1 || N < 1) return 0;
  return (size_t)P * N * (2 * sizeof(double) + sizeof(int));
}

extern "C" int fdipt_sample_lddt(const FdiptLddtArgs* a, fdipt_stream_t stream) {
  const int rc = ld_check_args(a, a ? a->score_mask : nullptr);
  if (rc != FDIPT_OK) return rc;
  const long tiles = cdiv(a->N, FD_WAVES), K = ld_set_atoms(a->mode);
  if (a->workspace_bytes < fdipt_sample_lddt_workspace(a->P, a->N)) return FDIPT_ESIZE;
  const dim3 grid((unsigned)(tiles * a->P)), block(FD_THREADS);
  if (a->mode == FDIPT_LDDT_CA)
    hipLaunchKernelGGL((lddt_pair_kernel<1, FDIPT_LDDT_TILE>), grid, block, 0, (hipStream_t)stream, *a, (int)tiles);
  else if (a->mode == FDIPT_LDDT_BACKBONE)
    hipLaunchKernelGGL((lddt_pair_kernel<4, FDIPT_LDDT_TILE>), grid, block, 0, (hipStream_t)stream, *a, (int)tiles);
  else
    hipLaunchKernelGGL((lddt_pair_kernel<37, FDIPT_LDDT_TILE_ALL>), grid, block, 0, (hipStream_t)stream, *a, (int)tiles);
  FD_CHECK_LAUNCH();
  hipLaunchKernelGGL(lddt_reduce_kernel, dim3(a->P), block, 0, (hipStream_t)stream, *a, (int)K);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
