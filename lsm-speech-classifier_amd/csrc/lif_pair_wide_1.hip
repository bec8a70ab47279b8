// Pair-block ring LIF kernel instantiations for 129..256 input channels (INMASK 3: bit planes) with 1 block(s)
// (= 2 neurons per lane) per wave (see lif_pair.h).
#include "lif_pair.h"

namespace lsm_lif {
pair_fn_t pick_pair_wide_1(int wpc, bool leakv, bool state) { return pick_pair_wide<1>(wpc, leakv, state); }
}  // namespace lsm_lif
