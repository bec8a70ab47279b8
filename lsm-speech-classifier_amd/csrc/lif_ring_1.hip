// Ring-row LIF kernel instantiations with 1 quad(s) (= 4 neurons per lane) per wave (see lif_ring.h).
#include "lif_ring.h"

namespace lsm_lif {
ring_fn_t pick_ring_1(int wpc, bool inreg, bool strided, bool state) { return pick_ring<1>(wpc, inreg, strided, state); }
ring_fn_t pick_ring_mask_1(int wpc, int inmask, bool state) { return pick_ring_mask<1>(wpc, inmask, state); }
}  // namespace lsm_lif
