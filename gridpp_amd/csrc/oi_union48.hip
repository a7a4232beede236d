// k_oi_union with 48 register columns (max_points 33..48; round 6): its own translation unit so that it compiles beside oi.hip and oi_union64.hip.
#include "oi_union.h"

void gpp_launch_union48(const OiArgs& a, const unsigned nblocks, const bool plain, const bool list, hipStream_t stream) {
    static constexpr void (*forms[2][2])(OiArgs) = {{k_oi_union<true, true, 48>, k_oi_union<true, false, 48>}, {k_oi_union<false, true, 48>, k_oi_union<false, false, 48>}};   // forms[not plain][not list]
    gpp::launch_on(stream, forms[plain ? 0 : 1][list ? 0 : 1], nblocks, 64 * UnionCfg<48>::WPB, 0, a);
}
