// pair_k9.hip - instantiates the fused contact kernels (contact_kernel) of the fixed-cutoff search kinds; see contact_kernels.hpp.
#include "contact_kernels.hpp"

namespace mh {

void launch_contacts(int kind, unsigned num_cus, hipStream_t stream, const pairk::SearchParams *dP, const pairk::SlotDesc *slot_desc,
                     uint32_t nslots, const pairk::ContactArgs &A) {
    using namespace pairk;
    if (kind == MOLAR_HIP_SEARCH_SINGLE) launch_contact_kernel<MOLAR_HIP_SEARCH_SINGLE>(num_cus, stream, dP, slot_desc, nslots, A);
    else launch_contact_kernel<MOLAR_HIP_SEARCH_DOUBLE>(num_cus, stream, dP, slot_desc, nslots, A);
}

}  // namespace mh
