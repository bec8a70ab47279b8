// LIF kernel instantiations with INREG=0, SEGLDS=0 (see lif_kernel.h); one translation unit
// per combination so that the four build in parallel.
#include "lif_kernel.h"

namespace lsm_lif {
lif_fn_t pick_lif_00(int sl, int wpc, bool state) { return pick_sl<false, false>(sl, wpc, state); }
}  // namespace lsm_lif
