// Pair-block ring LIF kernel instantiations with 3 block(s) (= 6 neurons per lane) per wave (see lif_pair.h).
#include "lif_pair.h"

namespace lsm_lif {
pair_fn_t pick_pair_3(int wpc, int inmask, bool leakv, bool state) { return pick_pair<3>(wpc, inmask, leakv, state); }
}  // namespace lsm_lif
