// Pair-block ring LIF kernel instantiations for 129..256 input channels (INMASK 3: bit planes) with 3 block(s)
// (= 6 neurons per lane) per wave (see lif_pair.h).
#include "lif_pair.h"

namespace lsm_lif {
pair_fn_t pick_pair_wide_3(int wpc, bool leakv, bool state) { return pick_pair_wide<3>(wpc, leakv, state); }
}  // namespace lsm_lif
