// pair_table.hip -- one evaluation order's launchers (pair_launchers.h) gathered into the table dispatch.cpp routes through.
// Host code only; compiled once per evaluation order of the point-mass term (pair_ns.h), like the units that define the launchers.
#include "pair_ns.h"

namespace eph {
namespace EPH_PV_NS {

// the table dispatch.cpp routes through (one per evaluation order). A function-local static: a namespace-scope const
// aggregate would be emitted for the device as well, where host functions do not exist.
const PairKernels *pair_table() {
    static const PairKernels t = {accel_wave,      accel_wg,   lm_step_wave,      lm_step_wg,   lm_persistent, lm_small,    lm_small_many,
                                  lm_double_small, srkn_small, srkn_double_small, srkn_small_many, srkn_double_small_many,
                                  lm_startup_small, lm_startup_small_many,
                                  lm_step_fast,    craft_launch, kPairVariant};
    return &t;
}

}  // namespace EPH_PV_NS
}  // namespace eph
