// pair_k11.hip - the count and fill kernels of distance_search_double(_pbc) for plans whose slots are cut from live rows
// (pair_kernel<KIND, MODE, 0, LIVE = true>, see pair_kernels.hpp and search_shape.hpp, live_row_slots).
#include "pair_kernels.hpp"

namespace mh {

void launch_pair_double_live(int mode, unsigned nblocks, hipStream_t stream, const pairk::SearchParams *dP,
                             const pairk::SlotDesc *slot_desc, uint32_t nslots, uint32_t *slot_cnt,
                             const unsigned long long *slot_base, uint2 *pairs, float *dist) {
    using namespace pairk;
    constexpr int KIND = MOLAR_HIP_SEARCH_DOUBLE;
    if (mode == MODE_COUNT)
        launch_pair_kernel<KIND, MODE_COUNT, 0, true>(nblocks, 0, stream, dP, slot_desc, nslots, slot_cnt, slot_base, pairs, dist, nullptr);
    else
        launch_pair_kernel<KIND, MODE_FILL, 0, true>(nblocks, 0, stream, dP, slot_desc, nslots, slot_cnt, slot_base, pairs, dist, nullptr);
}

}  // namespace mh
