// The row segments of a marching kernel's launch (k_box_march / k_minmax_march, k_score_march, k_fss_march): a plane of Y rows goes in `segs` segments of SH rows
// each, SH a whole number of the kernel's chunks.  The caller says how many segments it wants (from the workgroups it aims for and the strips and planes it has);
// the field may have fewer chunks than that, and gridDim.y is a 16-bit quantity.  Standard library only: tests/cpp/test_march_geom.cpp holds it against the three
// formulas it replaced.
#pragma once
#include <algorithm>

namespace gpp {

struct MarchSegments { int SH, segs; };

inline MarchSegments march_segments(int Y, int chunk, long want) {
    const int even = (int)std::max<long>(1, std::min<long>(want, (Y + chunk - 1) / chunk));
    int SH = ((Y + even - 1) / even + chunk - 1) / chunk * chunk;
    while((Y + SH - 1) / SH > 65535) SH += chunk;
    return {SH, (Y + SH - 1) / SH};
}

}   // namespace gpp
