// The reusable OI gain (include/gridpp_hip.h: gpp_oi_gain_*).  For every background point the observations the reference
// would select (src/api/oi.cpp:229-287), their weights w = G (P + R)^-1 (:315-317) and a = w . g (:336-337) are computed ONCE per
// geometry; an analysis is then increment = w . (obs - background_at_points) per cell and field, a gather and a dot product.
//
// Planes (all of them in tiles of 64 cells, the tiles of k_oi: gpp_tile_wshift for a grid, 64 consecutive points otherwise):
//   idx  int32   [tile][slot][64]   observation index in the caller's order, ascending within a cell; -1 behind the selection
//   w    double  [tile][slot][64]   the weight of that observation; 0 behind the selection
//   a    double  [tile][64]         w . g
//   cnt  uint8   [tile][64]         selected observations of the cell
// Slot-major inside a tile: with a cell per lane (k_oi_gain_apply, few fields) a wave reads 512 contiguous bytes per slot; with a
// field per lane (k_oi_gain_apply_wide) a workgroup reads the one contiguous block of its tile.
#include "oi_common.h"
#include <climits>
#include <memory>

using namespace gpp;

void gpp_oi_drain_pending();   // oi.hip: the deferred calls of this thread share the structure-field workspace with a build

namespace {
struct GainMap {   // background point <-> (tile, lane)
    int C, ny, nx, tiled2d, wshift, tiles_x, ntiles, K;
};
__device__ __forceinline__ int gain_cell(const GainMap& m, const int tile, const int lane) {
    if(m.tiled2d) {
        const int ty = tile / m.tiles_x, tx = tile - ty * m.tiles_x;
        const int y = ty * (64 >> m.wshift) + (lane >> m.wshift), x = (tx << m.wshift) + (lane & ((1 << m.wshift) - 1));
        return (y < m.ny && x < m.nx) ? y * m.nx + x : -1;
    }
    const int c = tile * 64 + lane;
    return c < m.C ? c : -1;
}
struct GainBuildArgs {
    ScanArgs s;
    GainMap m;
    const float *gx, *gy, *gz, *gelev, *glaf;
    const float4* ogeo;   // observations in the caller's order: x, y, z, elev
    const float4* oaux;   // laf, -, -, ratio
    int* idx; double* w; double* a; unsigned char* cnt;
    int* status;          // [0] error bits (2: singular), [1] largest selection
};
constexpr int GAIN_ERR_SINGULAR = 2;
constexpr int APPLY_WIDE_MIN_FIELDS = 16;   // from this many fields on the lanes of a wave run along the fields (k_oi_gain_apply_wide)
}   // namespace

// Selection and weights of one tile per wave.  The scan is scan_tile with the arguments of k_oi; the selections of the tile are sorted by
// observation index, the cells with the same selection form a group, and a group costs ONE inversion of (P + R) -- Gauss-Jordan with row
// pivoting in double, row i of the matrix in lane i, the matrix in LDS, which is what arma::inv does for the reference -- and a
// vector-matrix product per cell.  An exactly zero pivot column raises the singular bit.
template <int N, bool PLAIN>
__global__ __launch_bounds__(64) void k_oi_gain_build(GainBuildArgs a) {
    __shared__ unsigned long long s_a[N][64];   // the keys of the scan; then rows [0, N/2) the sorted index lists (u32), rows [N/2, N) their rho (f32)
    __shared__ double s_m[N][64];               // the sorted keys on their way; then the matrix of a group
    const int lane = threadIdx.x;
    d_exptab_fill<64>();
    __syncthreads();
    const int tile = blockIdx.x;
    const int cell = gain_cell(a.m, tile, lane);
    float gx = 0, gy = 0, gz = 0, ge = NAN, gl = NAN;
    if(cell >= 0) { gx = a.gx[cell]; gy = a.gy[cell]; gz = a.gz[cell]; ge = a.gelev[cell]; gl = a.glaf[cell]; }
    const bool active = cell >= 0;
    unsigned long long (*keys)[64] = s_a;
    DevStructure cst = a.s.st;   // this lane's structure: uniform, or the parameters at its background point
    if(cst.fh && cell >= 0) d_structure_at(cst, cst.cell_idx ? cst.cell_idx[cell] : cell);
    bool overflow, truncated;
    int cnt = scan_tile<N, false, PLAIN, false, true>(a.s, cst, active, gx, gy, gz, ge, gl, keys, lane, overflow, truncated);
    cnt = active ? cnt : 0;
    const int maxc = (int)wave_max((float)cnt);

    // ---- every lane's selection in ascending observation order (the indices of a cell are unique: rank = position) ----
    unsigned long long (*srt)[64] = reinterpret_cast<unsigned long long (*)[64]>(&s_m[0][0]);
    for(int s = 0; s < maxc; ++s) {
        const unsigned long long ks = keys[s][lane];
        const unsigned os = ~(unsigned)(ks & 0xffffffffull);
        int r = 0;
        for(int t = 0; t < maxc; ++t) {
            const unsigned ot = ~(unsigned)(keys[t][lane] & 0xffffffffull);
            r += (t < cnt && ot < os) ? 1 : 0;
        }
        if(s < cnt) srt[r][lane] = ks;
    }
    wave_lds_sync();
    unsigned (*origs)[64] = reinterpret_cast<unsigned (*)[64]>(&s_a[0][0]);
    float (*rho)[64] = reinterpret_cast<float (*)[64]>(&s_a[N / 2][0]);
    for(int s = 0; s < maxc; ++s) {
        if(s < cnt) {
            const unsigned long long k = srt[s][lane];
            origs[s][lane] = ~(unsigned)(k & 0xffffffffull);
            rho[s][lane] = __uint_as_float((unsigned)(k >> 32));
        }
    }
    wave_lds_sync();

    const size_t pbase = (size_t)tile * a.m.K * 64 + lane;
    for(int s = 0; s < a.m.K; ++s) {
        a.idx[pbase + (size_t)s * 64] = s < cnt ? (int)origs[s][lane] : -1;
        a.w[pbase + (size_t)s * 64] = 0.0;
    }
    a.cnt[(size_t)tile * 64 + lane] = (unsigned char)cnt;
    a.a[(size_t)tile * 64 + lane] = 0.0;
    if(lane == 0 && maxc > 0) atomicMax(a.status + 1, maxc);

    // ---- one inversion per distinct selection ----
    double (*M)[64] = s_m;
    unsigned long long todo = wave_ballot(cnt > 0);
    bool bad = false;
    while(todo != 0ull) {
        const int l = (int)__builtin_ctzll(todo);
        const int n = __builtin_amdgcn_readlane(cnt, l);
        bool same = cnt == n;
        for(int s = 0; s < n; ++s) same = same && origs[s][lane] == origs[s][l];
        todo &= ~wave_ballot(same);
        // row i of P + R in lane i: corr(obs_i, obs_p) with the structure at obs_i (oi.cpp:304-312), R on the diagonal
        const unsigned orig_i = lane < n ? origs[lane][l] : 0u;
        float4 o0 = make_float4(0, 0, 0, NAN), o1 = make_float4(NAN, 0, 0, 0);
        if(lane < n) { o0 = a.ogeo[orig_i]; o1 = a.oaux[orig_i]; }
        DevStructure pst = a.s.st;
        if(pst.fh && lane < n) d_structure_at(pst, pst.obs_idx[orig_i]);
        for(int p = 0; p < n; ++p) {
            const float xp = readlane_f(o0.x, p), yp = readlane_f(o0.y, p), zp = readlane_f(o0.z, p);
            const float ep = readlane_f(o0.w, p), lp = readlane_f(o1.x, p);
            const float c = d_corr_t<PLAIN, true>(pst, o0.x, o0.y, o0.z, o0.w, o1.x, xp, yp, zp, ep, lp, false);
            double v = (double)c;
            if(lane == p) v += (double)o1.w;
            M[p][lane] = lane < n ? v : 0.0;
        }
        wave_lds_sync();
        // In-place Gauss-Jordan.  Step k takes the unused row with the largest |entry| in column k (the lowest lane on a tie) as its pivot row
        // p_k, and slot k of every row then holds column p_k of the accumulated row operations E: at the end E (P + R) has its ones at
        // (p_k, k), i.e. (P + R)^-1[k][p_j] = slot j of lane p_k.  The other rows take the UNSCALED pivot row with the multiplier entry / pivot,
        // exactly 1 for an equal entry: two equal rows cancel exactly, and the column they leave empty is what raises the singular bit.
        int mystep = -1, mypiv = 0;
        for(int k = 0; k < n; ++k) {
            const double mk = M[k][lane];
            const double av = (lane < n && mystep < 0) ? fabs(mk) : -1.0;
            const double amax = wave_max_d(av);
            const int p = (int)__builtin_ctzll(wave_ballot(av == amax) | (1ull << 63));
            if(!(amax > 0.0)) bad = true;   // exactly singular (arma::inv throws)
            const double piv = readlane_d(mk, p);
            const double rp = 1.0 / piv;
            const double f = mk == piv ? 1.0 : mk * rp;   // (a row equal to the pivot row cancels exactly)
            if(lane == p) mystep = k;
            if(lane == k) mypiv = p;
            M[k][lane] = lane == p ? 1.0 : 0.0;
            wave_lds_sync();
            // (slot j of the pivot row is read by every lane in the instruction before the pivot lane overwrites it, and no other slot is
            //  touched in between: the slots are independent, and unrolled their LDS round trips overlap -- at one wave per SIMD nothing else hides them)
            for(int j0 = 0; j0 < n; j0 += 6) {
                double pr[6], mine[6];
#pragma unroll
                for(int u = 0; u < 6; ++u) { const int jj = min(j0 + u, n - 1); pr[u] = M[jj][p]; mine[u] = M[jj][lane]; }
#pragma unroll
                for(int u = 0; u < 6; ++u)
                    if(j0 + u < n) M[j0 + u][lane] = lane == p ? pr[u] * rp : __builtin_fma(-f, pr[u], mine[u]);
            }
            wave_lds_sync();
        }
        // the rows into the order of their steps: M[j][k] = (P + R)^-1[k][p_j]
        for(int j = 0; j < n; ++j) {
            const double v = M[j][lane];
            wave_lds_sync();
            if(lane < n && mystep >= 0) M[j][mystep] = v;
        }
        wave_lds_sync();
        // w = g (P + R)^-1 of every cell of the group (a cell per lane; g is the rho of its keys, oi.cpp:250), a = w . g
        double asum = 0.0;
        for(int j = 0; j < n; ++j) {
            const int pj = __builtin_amdgcn_readlane(mypiv, j);
            double acc = 0.0;
#pragma unroll 6
            for(int k = 0; k < n; ++k) acc = __builtin_fma((double)rho[k][lane], M[j][k], acc);
            if(same) {
                a.w[pbase + (size_t)pj * 64] = acc;
                asum = __builtin_fma(acc, (double)rho[pj][lane], asum);
            }
        }
        if(same) a.a[(size_t)tile * 64 + lane] = asum;
        __builtin_amdgcn_wave_barrier();
    }
    if(wave_ballot(bad) != 0ull && lane == 0) atomicOr(a.status, GAIN_ERR_SINGULAR);
}

// d = (double) pobs - (double) pbackground for every (station, field); flag[e]: the lowest usable station of field e with an invalid value
__global__ void k_oi_gain_innovation(const float* __restrict__ pobs, const int per_field, const float* __restrict__ pbg,
                                     const unsigned char* __restrict__ usable, const int S, const int E, double* __restrict__ d,
                                     int* __restrict__ flag) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= (long long)S * E) return;
    const int s = (int)(i / E), e = (int)(i - (long long)s * E);
    const float ob = pobs[per_field ? i : s], pb = pbg[i];
    d[i] = (double)ob - (double)pb;
    if(usable[s] && !(dev_valid(ob) && dev_valid(pb))) atomicMin(flag + e, s);
}

// the clamp of oi.cpp:318-334 on the float32 increment
__device__ __forceinline__ float gain_clamp(float increment, const float maxInc, const float minInc) {
    if(maxInc > 0 && increment > maxInc) increment = maxInc;
    else if(maxInc < 0 && increment > 0) increment = maxInc;
    else if(minInc < 0 && increment < minInc) increment = minInc;
    else if(minInc > 0 && increment < 0) increment = minInc;
    return increment;
}

// A cell per lane, a tile per wave: every slot of the planes is one contiguous 512-byte (w) and 256-byte (idx) read; the innovations come
// from the table in L2.  The form for few fields (the fields are an outer loop: the planes of the tile come from L1 / L2 again).
__global__ __launch_bounds__(256) void k_oi_gain_apply(const GainMap m, const int* __restrict__ idx, const double* __restrict__ w,
                                                       const unsigned char* __restrict__ cnt, const float* __restrict__ bg,
                                                       const double* __restrict__ d, const int E, const int allow_extrap, float* __restrict__ out) {
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if(tile >= m.ntiles) return;
    const int cell = gain_cell(m, tile, lane);
    if(cell < 0) return;
    const int n = cnt[(size_t)tile * 64 + lane];
    const size_t pbase = (size_t)tile * m.K * 64 + lane;
    for(int e = 0; e < E; ++e) {
        const float b = bg[(size_t)cell * E + e];
        float res = b;
        if(n > 0 && dev_valid(b)) {   // oi.cpp:223
            double acc = 0.0;
            float maxInc = -INFINITY, minInc = INFINITY;
            for(int k = 0; k < n; ++k) {
                const int i = idx[pbase + (size_t)k * 64];
                const double dv = d[(size_t)i * E + e];
                acc = __builtin_fma(w[pbase + (size_t)k * 64], dv, acc);
                const float df = (float)dv;
                maxInc = fmaxf(maxInc, df); minInc = fminf(minInc, df);
            }
            float increment = (float)acc;
            if(!allow_extrap) increment = gain_clamp(increment, maxInc, minInc);
            res = b + increment;
        }
        out[(size_t)cell * E + e] = res;
    }
}

// A field per lane, a tile per workgroup, sixteen cells per wave.  The workgroup first copies the planes of its tile -- one contiguous
// block of K * 64 weights, one of K * 64 indices, 64 counts -- into LDS with every load in flight at once; read per cell from HBM, one
// strided gather after the other behind the count they depend on, they were three dependent HBM round trips per cell and wave.  Lane k
// then takes slot k of a cell from LDS ONCE (index and weight stay in two registers of the wave and are broadcast with v_readlane).  The
// fields of a cell are contiguous in the background, in the result and in the innovation table (gridpp's cube layout, E innermost), so
// every access of the field loop is one contiguous run of E values; the background of the next cell is asked for before this one's
// slots are walked.  The slots are taken eight at a time: eight independent reads of the table in flight per lane instead of one round
// trip per slot.  A slot behind the selection repeats the cell's first observation with weight 0 (a usable station: its innovation is
// finite).  Dynamic LDS: K * 64 * 12 + 256 bytes.
template <bool EXTRAP>
__global__ __launch_bounds__(256) void k_oi_gain_apply_wide(const GainMap m, const int* __restrict__ idx, const double* __restrict__ w,
                                                            const unsigned char* __restrict__ cnt, const float* __restrict__ bg,
                                                            const double* __restrict__ d, const int E, float* __restrict__ out) {
    extern __shared__ double s_w[];   // [K][64] weights, [K][64] indices, [64] counts
    int* const s_idx = reinterpret_cast<int*>(s_w + (size_t)m.K * 64);
    int* const s_cnt = s_idx + (size_t)m.K * 64;
    const int tile = blockIdx.x, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t tbase = (size_t)tile * m.K * 64;
    for(int q = threadIdx.x; q < m.K * 64; q += 256) { s_w[q] = w[tbase + q]; s_idx[q] = idx[tbase + q]; }
    if(threadIdx.x < 64) s_cnt[threadIdx.x] = cnt[(size_t)tile * 64 + threadIdx.x];
    __syncthreads();
    for(int e0 = 0; e0 < E; e0 += 64) {
        const int e = min(e0 + lane, E - 1);
        int cell = gain_cell(m, tile, wv * 16);
        float b = cell >= 0 ? bg[(size_t)cell * E + e] : 0.0f;
        for(int c = wv * 16; c < wv * 16 + 16; ++c) {
            const int cell_next = c + 1 < wv * 16 + 16 ? gain_cell(m, tile, c + 1) : -1;
            const float b_next = cell_next >= 0 ? bg[(size_t)cell_next * E + e] : 0.0f;
            if(cell >= 0) {
                const int n = s_cnt[c];
                const int ls = lane < n ? lane : 0;
                const int il = n > 0 ? s_idx[ls * 64 + c] * E : 0;   // (row of the table: stations x fields < 2^31)
                const double wl = lane < n ? s_w[ls * 64 + c] : 0.0;
                double acc = 0.0;
                float maxInc = -INFINITY, minInc = INFINITY;
                for(int k0 = 0; k0 < n; k0 += 8) {
                    double dv[8];
#pragma unroll
                    for(int u = 0; u < 8; ++u) dv[u] = d[__builtin_amdgcn_readlane(il, k0 + u) + e];
#pragma unroll
                    for(int u = 0; u < 8; ++u) {
                        acc = __builtin_fma(readlane_d(wl, k0 + u), dv[u], acc);
                        if(!EXTRAP) {
                            const float df = (float)dv[u];
                            maxInc = k0 + u < n ? fmaxf(maxInc, df) : maxInc; minInc = k0 + u < n ? fminf(minInc, df) : minInc;
                        }
                    }
                }
                float increment = (float)acc;
                if(!EXTRAP) increment = gain_clamp(increment, maxInc, minInc);
                const float res = (n > 0 && dev_valid(b)) ? b + increment : b;
                if(e0 + lane < E) out[(size_t)cell * E + e] = res;
            }
            cell = cell_next; b = b_next;
        }
    }
}

// out = bvariance (1 - a) where the cell has a selection (oi.cpp:336-337), bvariance elsewhere
__global__ __launch_bounds__(256) void k_oi_gain_variance(const GainMap m, const double* __restrict__ a, const unsigned char* __restrict__ cnt,
                                                          const float* __restrict__ bvar, float* __restrict__ out) {
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if(tile >= m.ntiles) return;
    const int cell = gain_cell(m, tile, lane);
    if(cell < 0) return;
    const float bv = bvar[cell];
    const size_t t = (size_t)tile * 64 + lane;
    out[cell] = cnt[t] > 0 ? (float)((double)bv * (1.0 - a[t])) : bv;
}

// the planes in the caller's cell order: counts[cell], indices[cell][K], weights[cell][K]
__global__ __launch_bounds__(256) void k_oi_gain_unpack(const GainMap m, const int* __restrict__ idx, const double* __restrict__ w,
                                                        const unsigned char* __restrict__ cnt, int* __restrict__ counts, int* __restrict__ indices,
                                                        double* __restrict__ weights) {
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if(tile >= m.ntiles) return;
    const int cell = gain_cell(m, tile, lane);
    if(cell < 0) return;
    if(counts) counts[cell] = cnt[(size_t)tile * 64 + lane];
    const size_t pbase = (size_t)tile * m.K * 64 + lane;
    for(int k = 0; k < m.K; ++k) {
        if(indices) indices[(size_t)cell * m.K + k] = idx[pbase + (size_t)k * 64];
        if(weights) weights[(size_t)cell * m.K + k] = w[pbase + (size_t)k * 64];
    }
}

struct gpp_oi_gain {
    GainMap m = GainMap();
    int S = 0, largest = 0;
    DevBuf<int> idx;
    DevBuf<double> w, a;
    DevBuf<unsigned char> cnt, usable;
    DevBuf<double> d;      // the innovation table of the last apply (S x E doubles): the gain's own, no workspace slot of the OI calls
    DevBuf<int> flag;
    size_t plane() const { return (size_t)m.ntiles * m.K * 64; }
    size_t cells64() const { return (size_t)m.ntiles * 64; }
    long long bytes() const {
        return (long long)(idx.cap * sizeof(int) + (w.cap + a.cap + d.cap) * sizeof(double) + cnt.cap + usable.cap + flag.cap * sizeof(int));
    }
};

extern "C" int gpp_oi_gain_create(gpp_points* bgrid, gpp_points* points, const float* pratios, const unsigned char* usable,
                                  const gpp_structure* st, int max_points, gpp_oi_gain** gain) {
    GPP_TRY
    if(!bgrid || !points || !gain) invalid("grid/points/gain handle is NULL");
    if(bgrid->type != points->type)
        invalid("Both background and observations points must be of same coordinate type (lat/lon or x/y)");
    if(max_points < 1) invalid("max_points must be >= 1: a gain holds max_points columns per background point");
    if(max_points > GPP_OI_GAIN_MAX_POINTS) invalid("max_points must be <= " + std::to_string(GPP_OI_GAIN_MAX_POINTS) + " (GPP_OI_GAIN_MAX_POINTS)");
    if(points->n > 0 && !pratios) invalid("pratios is NULL");
    if(!st) invalid("structure is NULL");
    ensure_device();
    gpp_oi_drain_pending();
    const int C = bgrid->n, S = points->n;
    std::unique_ptr<gpp_oi_gain> g(new gpp_oi_gain);
    GainMap& m = g->m;
    m.C = C; m.ny = bgrid->ny; m.nx = bgrid->nx; m.K = max_points;
    m.tiled2d = (bgrid->nx > 0 && (long)bgrid->ny * bgrid->nx == C) ? 1 : 0;
    m.wshift = 3;
    if(m.tiled2d) {
        m.wshift = gpp_tile_wshift(bgrid);
        const int tw = 1 << m.wshift, th = 64 >> m.wshift;
        m.tiles_x = (m.nx + tw - 1) / tw; m.ntiles = m.tiles_x * ((m.ny + th - 1) / th);
    }
    else { m.tiles_x = 0; m.ntiles = (C + 63) / 64; }
    g->S = S;
    // an empty gain: no selection anywhere (no background points, no observations, or none of them usable)
    std::vector<unsigned char> us(std::max(S, 1), 1);
    int nusable = S;
    if(usable) { nusable = 0; for(int i = 0; i < S; i++) { us[i] = usable[i] ? 1 : 0; nusable += us[i]; } }
    g->usable.upload(us.data(), (size_t)S);
    g->idx.get(g->plane()); g->w.get(g->plane()); g->a.get(g->cells64()); g->cnt.get(g->cells64());
    if(C == 0 || nusable == 0) {
        if(g->plane()) {
            GPP_HIP(hipMemsetAsync(g->idx.p, 0xFF, g->plane() * sizeof(int), stream()));
            GPP_HIP(hipMemsetAsync(g->w.p, 0, g->plane() * sizeof(double), stream()));
            GPP_HIP(hipMemsetAsync(g->a.p, 0, g->cells64() * sizeof(double), stream()));
            GPP_HIP(hipMemsetAsync(g->cnt.p, 0, g->cells64(), stream()));
        }
        GPP_HIP(hipStreamSynchronize(stream()));
        *gain = g.release();
        return GPP_OK;
    }
    // the bin-sorted observation block of the OI calls (k_pack_obs): an unusable station has an invalid "observation"
    bgrid->to_device();
    gpp_obs_index* ix = gpp_build_obs_index(points);
    std::vector<float> ob(S);
    for(int i = 0; i < S; i++) ob[i] = us[i] ? 0.0f : NAN;
    DevBuf<float> d_ob, d_ratio;
    DevBuf<float4> pgeo, oaux;
    DevBuf<int> status, cbuf, obuf;
    d_ob.upload(ob.data(), S); d_ratio.upload(pratios, S);
    pgeo.get(S); oaux.get(S); status.get(2);
    GPP_HIP(hipMemsetAsync(status.p, 0, 2 * sizeof(int), stream()));
    launch(k_pack_obs, blocks_of(S), 256, 0, S, ix->d_sgeo.p, ix->d_pos.p, ix->d_olaf.p, d_ob.p, d_ratio.p,
           (const float*)nullptr, (const float*)nullptr, 0, pgeo.p, oaux.p, (float4*)nullptr, (unsigned long long*)nullptr, 0);
    GainBuildArgs a = GainBuildArgs();
    const int N = max_points <= 32 ? 32 : 62;
    gpp_scan_geometry(a.s, ix, S, max_points, N);
    a.s.pgeo = pgeo.p; a.s.scan_stats = nullptr;
    a.s.st = gpp_resolve_structure(st);
    gpp_bind_field(a.s.st, st, bgrid, points, cbuf, obuf);
    a.m = m;
    a.gx = bgrid->d_x.p; a.gy = bgrid->d_y.p; a.gz = bgrid->d_z.p; a.gelev = bgrid->d_elev.p; a.glaf = bgrid->d_laf.p;
    a.ogeo = ix->d_ogeo.p; a.oaux = oaux.p;
    a.idx = g->idx.p; a.w = g->w.p; a.a = g->a.p; a.cnt = g->cnt.p; a.status = status.p;
    const bool plain = a.s.st.kh == GPP_SK_BARNES && a.s.st.kv == GPP_SK_BARNES && a.s.st.kw == GPP_SK_BARNES && !a.s.st.cv;
    static constexpr void (*forms[2][2])(GainBuildArgs) = {{k_oi_gain_build<32, true>, k_oi_gain_build<32, false>}, {k_oi_gain_build<62, true>, k_oi_gain_build<62, false>}};
    launch(forms[N != 32][plain ? 0 : 1], (unsigned)m.ntiles, 64, 0, a);
    int h_status[2] = {0, 0};
    GPP_HIP(hipMemcpyAsync(h_status, status.p, sizeof(h_status), hipMemcpyDeviceToHost, stream()));
    GPP_HIP(hipStreamSynchronize(stream()));
    if(h_status[0] & GAIN_ERR_SINGULAR) runtime("optimal_interpolation_gain: local (P+R) matrix is singular");
    g->largest = h_status[1];
    *gain = g.release();
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_oi_gain_destroy(gpp_oi_gain* gain) {
    GPP_TRY
    delete gain;
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_oi_gain_info(const gpp_oi_gain* gain, long long* cells, int* stations, int* max_points, long long* bytes, int* largest) {
    GPP_TRY
    if(!gain) invalid("gain handle is NULL");
    if(cells) *cells = gain->m.C;
    if(stations) *stations = gain->S;
    if(max_points) *max_points = gain->m.K;
    if(bytes) *bytes = gain->bytes();
    if(largest) *largest = gain->largest;
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_oi_gain_apply(gpp_oi_gain* gain, const float* background, int ne, const float* pobs, int pobs_per_field,
                                 const float* pbackground, int allow_extrapolation, float* out, int mem) {
    GPP_TRY
    if(!gain) invalid("gain handle is NULL");
    if(ne < 1) invalid("ne must be >= 1");
    const int C = gain->m.C, S = gain->S;
    if(C > 0 && (!background || !out)) invalid("background/out is NULL");
    if(S > 0 && (!pobs || !pbackground)) invalid("observation arrays are NULL");
    if((long long)S * ne > (long long)INT_MAX) invalid("stations x fields must be below 2^31");
    ensure_device();
    if(C == 0) return GPP_OK;
    mem &= ~GPP_ASYNC;
    const size_t n = (size_t)C * ne;
    InField f_bg, f_obs, f_pbg;
    OutField f_out;
    f_bg.bind(background, n, mem);
    f_out.bind(out, n, mem);
    if(S == 0) {
        GPP_HIP(hipMemcpyAsync(f_out.d, f_bg.d, n * sizeof(float), hipMemcpyDeviceToDevice, stream()));
        return finish_call(f_out);
    }
    f_obs.bind(pobs, pobs_per_field ? (size_t)S * ne : (size_t)S, mem);
    f_pbg.bind(pbackground, (size_t)S * ne, mem);
    gain->d.get((size_t)S * ne); gain->flag.get(ne);
    GPP_HIP(hipMemsetAsync(gain->flag.p, 0x7f, (size_t)ne * sizeof(int), stream()));
    launch(k_oi_gain_innovation, blocks_of((size_t)S * ne), 256, 0, f_obs.d, pobs_per_field ? 1 : 0, f_pbg.d, (const unsigned char*)gain->usable.p, S, ne, gain->d.p, gain->flag.p);
    std::vector<int> flag(ne);
    GPP_HIP(hipMemcpyAsync(flag.data(), gain->flag.p, (size_t)ne * sizeof(int), hipMemcpyDeviceToHost, stream()));
    GPP_HIP(hipStreamSynchronize(stream()));
    for(int e = 0; e < ne; e++)
        if(flag[e] < S)
            invalid("optimal_interpolation_gain: pobs or pbackground is invalid at usable station " + std::to_string(flag[e]) + " of field " +
                    std::to_string(e) + " (mark the station unusable when the gain is built)");
    if(ne >= APPLY_WIDE_MIN_FIELDS) {
        const size_t lds = (size_t)gain->m.K * 64 * (sizeof(double) + sizeof(int)) + 64 * sizeof(int);
        launch(allow_extrapolation ? k_oi_gain_apply_wide<true> : k_oi_gain_apply_wide<false>, (unsigned)gain->m.ntiles, 256, lds, gain->m, (const int*)gain->idx.p,
               (const double*)gain->w.p, (const unsigned char*)gain->cnt.p, f_bg.d, (const double*)gain->d.p, ne, f_out.d);
    }
    else
        launch(k_oi_gain_apply, (gain->m.ntiles + 3) / 4, 256, 0, gain->m, (const int*)gain->idx.p, (const double*)gain->w.p, (const unsigned char*)gain->cnt.p,
               f_bg.d, (const double*)gain->d.p, ne, allow_extrapolation ? 1 : 0, f_out.d);
    return finish_call(f_out);
    GPP_CATCH
}

extern "C" int gpp_oi_gain_variance(gpp_oi_gain* gain, const float* bvariance, float* out, int mem) {
    GPP_TRY
    if(!gain) invalid("gain handle is NULL");
    const int C = gain->m.C;
    if(C > 0 && (!bvariance || !out)) invalid("bvariance/out is NULL");
    ensure_device();
    if(C == 0) return GPP_OK;
    mem &= ~GPP_ASYNC;
    InField f_bv;
    OutField f_out;
    f_bv.bind(bvariance, C, mem);
    f_out.bind(out, C, mem);
    launch(k_oi_gain_variance, (gain->m.ntiles + 3) / 4, 256, 0, gain->m, (const double*)gain->a.p, (const unsigned char*)gain->cnt.p, f_bv.d, f_out.d);
    return finish_call(f_out);
    GPP_CATCH
}

extern "C" int gpp_oi_gain_selection(gpp_oi_gain* gain, int* counts, int* indices, double* weights, int mem) {
    GPP_TRY
    if(!gain) invalid("gain handle is NULL");
    ensure_device();
    const size_t C = (size_t)gain->m.C, K = (size_t)gain->m.K;
    if(C == 0) return GPP_OK;
    const bool dev = (mem & GPP_MEM_DEVICE) != 0;
    DevBuf<int> t_counts, t_indices;
    DevBuf<double> t_weights;
    int* dc = counts ? (dev ? counts : t_counts.get(C)) : nullptr;
    int* di = indices ? (dev ? indices : t_indices.get(C * K)) : nullptr;
    double* dw = weights ? (dev ? weights : t_weights.get(C * K)) : nullptr;
    launch(k_oi_gain_unpack, (gain->m.ntiles + 3) / 4, 256, 0, gain->m, (const int*)gain->idx.p, (const double*)gain->w.p, (const unsigned char*)gain->cnt.p, dc, di, dw);
    if(!dev) {
        if(counts) GPP_HIP(hipMemcpyAsync(counts, dc, C * sizeof(int), hipMemcpyDeviceToHost, stream()));
        if(indices) GPP_HIP(hipMemcpyAsync(indices, di, C * K * sizeof(int), hipMemcpyDeviceToHost, stream()));
        if(weights) GPP_HIP(hipMemcpyAsync(weights, dw, C * K * sizeof(double), hipMemcpyDeviceToHost, stream()));
    }
    GPP_HIP(hipStreamSynchronize(stream()));
    return GPP_OK;
    GPP_CATCH
}
