// Ring-row LIF kernel instantiations with 2 quad(s) (= 8 neurons per lane) per wave (see lif_ring.h).
#include "lif_ring.h"

namespace lsm_lif {
ring_fn_t pick_ring_2(int wpc, bool inreg, bool strided, bool state) { return pick_ring<2>(wpc, inreg, strided, state); }
ring_fn_t pick_ring_mask_2(int wpc, int inmask, bool state) { return pick_ring_mask<2>(wpc, inmask, state); }
}  // namespace lsm_lif
