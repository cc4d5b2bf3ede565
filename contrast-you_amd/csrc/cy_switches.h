// The environment switches of the conv and weight-gradient code (A/B measurements and tests), in one table.
// Read together at the first use of any of them -- not at library load: a host program may set them between loading
// the library and its first call (tests/conftest.py sets CY_DGRAD_BN_ALL that way).  One instance per shared object:
// cy_switches() is an inline function with hidden visibility, so every translation unit sees the same static.
#pragma once
#include <cstdlib>

namespace cy_env {
static inline int as_int(const char* name, int dflt) {  // atoi of the value
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
static inline bool unless_0(const char* name) {  // on unless the value begins with '0'
  const char* e = getenv(name);
  return !(e && e[0] == '0');
}
}  // namespace cy_env

struct CySwitches {
  // per switch: the variable, its parsing (as_int: atoi, with the default when unset; unless_0: on by default, off
  // when the value begins with '0') and what the non-default values select
  bool conv_plane = cy_env::unless_0("CY_CONV_PLANE");           // =0: conv3x3_igemm_kernel for every width
  int stream = cy_env::as_int("CY_STREAM", 1);                   // =0: no streaming kernel on the 224^2 level; =2: no tile-count threshold
  int flow = cy_env::as_int("CY_FLOW", 1);                       // =0: plane kernel instead of the flow conv kernel
  int flow_cfg = cy_env::as_int("CY_FLOW_CFG", 0);               // =1..4: force one flow tiling (flow_apply_cfg in cy_conv3x3.hip)
  int plane_xcd = cy_env::as_int("CY_PLANE_XCD", 1);             // =0: tile = workgroup index (plane and flow kernels)
  int dgrad_bn_all = cy_env::as_int("CY_DGRAD_BN_ALL", 0);       // =1: lifts the launch-plan rule of the fused BatchNorm data gradient (tests)
  int bn_fold_in_kernel = cy_env::as_int("CY_BN_FOLD_IN_KERNEL", 1);  // =0: coefficients by a fold launch instead of in the consumer
  int first_mfma = cy_env::as_int("CY_FIRST_MFMA", 1);           // =0: VALU first layer
  bool first_wgrad_mfma = cy_env::unless_0("CY_FIRST_WGRAD_MFMA");  // =0: VALU first-layer weight gradient
  bool wgrad_spec = cy_env::unless_0("CY_WGRAD_SPEC");           // =0: wgrad12_kernel instead of the wave-specialised wgrad12s_kernel
  bool wgrad_dma = cy_env::unless_0("CY_WGRAD_DMA");             // =0: its loaders on register staging instead of LDS-DMA
  bool wgrad_blk = cy_env::unless_0("CY_WGRAD_BLK");             // =0: row-major k instead of its 4 x 4 patch order
};

__attribute__((visibility("hidden"))) inline const CySwitches& cy_switches() {
  static const CySwitches s{};
  return s;
}
