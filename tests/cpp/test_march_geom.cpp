// march_geom.h against the three formulas it replaced, restated here as they stood in neighbourhood.hip (MarchGeom), score.hip
// (gpp_neighbourhood_score) and fss.hip (FssCall::march): the same segment height and the same number of segments for every field
// height, strip count, plane count and fill target of the sweep.  No GPU, no HIP: built by tests/test_march_geom.py with g++ alone.
#include <algorithm>
#include <cstdio>

#include "march_geom.h"

namespace {

constexpr int CHUNK = 32;   // BM_C == SC_C == FS_C

struct Old { int SH, segs; };

// neighbourhood.hip, MarchGeom::MarchGeom
Old old_march_geom(int Y, int strips, int nplanes, long fill) {
    const int BM_C = CHUNK;
    int SH, segs;
    const long want = std::max<long>(1, fill / std::max<long>(1, (long)strips * nplanes));
    const int even = (int)std::min<long>(want, (Y + BM_C - 1) / BM_C);
    SH = ((Y + even - 1) / even + BM_C - 1) / BM_C * BM_C;
    while((Y + SH - 1) / SH > 65535) SH += BM_C;   // gridDim.y is a 16-bit quantity
    segs = (Y + SH - 1) / SH;
    return {SH, segs};
}

// score.hip, gpp_neighbourhood_score
Old old_score(int Y, int strips, long fill) {
    const int SC_C = CHUNK;
    const int segs = (int)std::max(1L, std::min((fill + strips - 1) / strips, (long)(Y + SC_C - 1) / SC_C));   // about a thousand workgroups where the field has them
    int SH = ((Y + segs - 1) / segs + SC_C - 1) / SC_C * SC_C;
    while((Y + SH - 1) / SH > 65535) SH += SC_C;
    return {SH, (Y + SH - 1) / SH};
}

// fss.hip, FssCall::march
Old old_fss(int Y, int strips, long fill) {
    const int FS_C = CHUNK;
    const int segs = (int)std::max(1L, std::min((fill + strips - 1) / strips, (long)(Y + FS_C - 1) / FS_C));
    int SH = ((Y + segs - 1) / segs + FS_C - 1) / FS_C * FS_C;
    while((Y + SH - 1) / SH > 65535) SH += FS_C;
    const int nseg = (Y + SH - 1) / SH;
    return {SH, nseg};
}

long failures = 0, cases = 0;

void check(const char* what, Old o, gpp::MarchSegments n, int Y, int strips, int nplanes, long fill) {
    cases++;
    if(o.SH == n.SH && o.segs == n.segs) return;
    if(failures++ < 20)
        std::printf("%s: Y %d strips %d planes %d fill %ld: parent SH %d segs %d, march_segments SH %d segs %d\n", what, Y, strips, nplanes, fill, o.SH, o.segs,
                    n.SH, n.segs);
}

void sweep(int Y) {
    const int planes[] = {1, 3, 100};
    const long fills[] = {1, 3, 768, 1024, 1280};
    for(int strips = 1; strips <= 70; strips++)
        for(long fill : fills) {
            // the callers' own `want`: MarchGeom rounds down, score and FSS round up
            for(int np : planes)
                check("MarchGeom", old_march_geom(Y, strips, np, fill), gpp::march_segments(Y, CHUNK, std::max<long>(1, fill / std::max<long>(1, (long)strips * np))), Y,
                      strips, np, fill);
            const long up = std::max(1L, (fill + strips - 1) / strips);
            check("score", old_score(Y, strips, fill), gpp::march_segments(Y, CHUNK, up), Y, strips, 1, fill);
            check("fss", old_fss(Y, strips, fill), gpp::march_segments(Y, CHUNK, up), Y, strips, 1, fill);
        }
}

}   // namespace

int main() {
    for(int Y = 1; Y <= 300; Y++) sweep(Y);
    const int more[] = {4000, 65535 * 32 - 1, 65535 * 32, 65535 * 32 + 1};
    for(int Y : more) sweep(Y);
    // a segment is whole chunks, and the segments cover the field with a 16-bit count
    for(int Y : more) {
        const gpp::MarchSegments s = gpp::march_segments(Y, CHUNK, 1L << 40);
        if(s.SH % CHUNK != 0 || s.segs > 65535 || (long)s.SH * s.segs < Y) { failures++; std::printf("Y %d: SH %d segs %d\n", Y, s.SH, s.segs); }
    }
    std::printf("%ld cases, %ld failures\n", cases, failures);
    if(failures) return 1;
    std::printf("all checks passed\n");
    return 0;
}
