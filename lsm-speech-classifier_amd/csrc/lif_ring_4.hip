// Ring-row LIF kernel instantiations with 4 quad(s) (= 16 neurons per lane) per wave (see lif_ring.h).
#include "lif_ring.h"

namespace lsm_lif {
ring_fn_t pick_ring_4(int wpc, bool inreg, bool strided, bool state) { return pick_ring<4>(wpc, inreg, strided, state); }
}  // namespace lsm_lif
