// k_oi_union with 64 register columns (max_points 33..62): its own translation unit so that it compiles beside oi.hip.
#include "oi_union.h"

void gpp_launch_union64(const OiArgs& a, const unsigned nblocks, const bool plain, const bool list, hipStream_t stream) {
    static constexpr void (*forms[2][2])(OiArgs) = {{k_oi_union<true, true, 64>, k_oi_union<true, false, 64>}, {k_oi_union<false, true, 64>, k_oi_union<false, false, 64>}};   // forms[not plain][not list]
    gpp::launch_on(stream, forms[plain ? 0 : 1][list ? 0 : 1], nblocks, 64 * UnionCfg<64>::WPB, 0, a);
}
