// gdt_mapped.hip — GDT-TS / GDT-HA of a model read through a row map (include/fdipt.h, "accuracy through a row map"; DESIGN.md section
// 7.16): fdipt_sample_gdt_mapped.  One launch, a block per pair: gdt_body.hpp's kernel in its MAPPED instantiation, which judges the
// pair's map first and compacts the CA atoms of (model row map[j], reference row j) for ascending j.
#include "gdt_body.hpp"

__global__ __launch_bounds__(FD_THREADS) void gdt_mapped_kernel(FdiptGdtArgs a, FdiptRowMap m) { gdt_body<true>(a, m); }

extern "C" int fdipt_sample_gdt_mapped(const FdiptGdtArgs* a, const FdiptRowMap* m, fdipt_stream_t stream) {
  if (!a || !m || a->S < 1 || a->N < 1 || a->P < 1 || m->N_a < 1) return FDIPT_EINVAL;
  if (!a->prot_b || !a->mask_b || a->S_b < 1) return FDIPT_EINVAL;
  for (int atoms : {a->atoms, a->atoms_b})
    if (atoms != 37 && atoms != 5 && atoms != 1) return FDIPT_EINVAL;
  // one CA column serves both structures: a CA trace goes with a CA trace
  if ((a->atoms == 1) != (a->atoms_b == 1) || a->ca < 0 || a->ca >= (a->atoms == 1 ? 1 : 5)) return FDIPT_EINVAL;
  if (a->mode != FDIPT_GDT_NONE && a->mode != FDIPT_GDT_GLOBAL && a->mode != FDIPT_GDT_SEARCH) return FDIPT_EINVAL;
  if (!a->prot || !a->mask || !a->pairs || !a->gdt_ts || !a->gdt_ha || !a->counts || !a->n_scored || !a->rotation || !a->translation || !a->best_item ||
      !a->best_pass || !a->passes || !a->res_within || !a->status || !m->map || !m->n_covered || !m->n_reference)
    return FDIPT_EINVAL;
  if (a->N > FDIPT_TM_MAX_ROWS || m->N_a > FDIPT_TM_MAX_ROWS) return FDIPT_ESIZE;
  const size_t lds = gdt_lds_bytes(a->N);
  static FdPerDevice attr_dev;
  const int dev_ = fd_device();
  if (!attr_dev.get(dev_)) {  // N = 1024: 131 KB, more than the default 64 KB of dynamic LDS
    if (hipFuncSetAttribute((const void*)gdt_mapped_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gdt_lds_bytes(FDIPT_TM_MAX_ROWS)) != hipSuccess)
      return FDIPT_ELAUNCH;
    attr_dev.set(dev_, 1);
  }
  hipLaunchKernelGGL(gdt_mapped_kernel, dim3((unsigned)a->P), dim3(FD_THREADS), lds, (hipStream_t)stream, *a, *m);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
