// smart_fast_steps.hip -- the step loops of the regular (class 0) rows: forcing that varies inside the report interval
// (genuinely sub-daily data: the asm arms of smart_fast_arms.h), raw reports, and report gaps of one step.  See
// smart_fast_entry.h for the family.
#include "smart_fast_entry.h"

namespace smart {

// (170 VGPRs: two wavefronts per SIMD.  An allocation bounded at 168 for a third was measured in round 6 and not kept:
// profiles/r06_ab_steps_third_wave.txt)
SMART_FAST_KERNEL(smart_fast_steps) { merged_kernel<FastModel<false, false, true>, kForcingVarying>(a, forcing, obs, ws); }

SMART_FAST_KERNEL(smart_fast_steps_states) { merged_kernel<FastModel<false, false, true, true, true>, kForcingVarying>(a, forcing, obs, ws); }

// raw reports / gap 1: the merged form when only discharge and the groundwater ratio are asked for, the five
// reservoirs carried separately when the caller wants the final state vector
SMART_FAST_KERNEL(smart_fast_plain)
{
    const Work w = claim_work(a, 0);
    if (!block_is_mine<0>(a, w))
        return;
    if (a.final_vars == nullptr)
        run_ensemble<FastModel<false, false, true>, false>(a, forcing, obs, ws, nullptr, w.block, w.c);
    else
        run_ensemble<FastModel<false, false>, false>(a, forcing, obs, ws, nullptr, w.block, w.c);
}

} // namespace smart
