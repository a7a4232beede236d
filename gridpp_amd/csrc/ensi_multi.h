// optimal_interpolation_ensi_multi_{ebe, ebesc, utem} (src/api/oi_ensi_multi.cpp:329-1311), included by ensi.hip.
//
// One 256-thread workgroup per grid point: radius query over the observation bins, LDS bitonic sort of the candidates (the
// prologue of k_ensi_big), then
//   ebe / ebesc : K = r (A + R)^-1 with A = C o (Z Z^T) (ebe: ensemble correlations Z localised by the static correlations C)
//                 or A = C (ebesc); pivoted LU in LDS on A^T (n <= 64 selected observations), then dx_e = ratio K innov_e for
//                 every member e (any number of members), the anti-extrapolation clamp, out = background + dx;
//   utem        : the E x E square-root filter of optimal_interpolation_ensi with Pinv = Yc^T Rinv Yc + I, Rinv = rho / pratio,
//                 W' = ensStd sqrt((E-1) P) + ratio w 1^T applied to the normalised perturbations of background_corr
//                 (E <= 64 valid members; any n up to the EBIG_CAND candidates of the LDS sort, 64 observations at a time).
// These functions have no performance configuration in BASELINE.json; the kernel is written for correctness first.
#pragma once

struct MultiArgs {
    EnsiArgs e;                 // gY = gZ (ebe) / gY_corr (utem); bg = background
    const float* gYm;           // utem: mean-removed pbackground of the valid members [S][nV]
    const float* bgc;           // background_corr [C][E] (ebe, utem)
    const float* bratios;       // [C]
    const float* pobs2;         // ebe / ebesc: [S][E]
    const float* pbg2;          // ebe / ebesc: [S][E]
    int oob;                    // an invalid member in front of a valid one: the reference indexes out of bounds
    int huge_ncap;              // k_ensi_multi_huge: most selected observations of a grid point (sizes its scratch)
    size_t huge_stride;         // doubles of scratch per workgroup
};

// calc_statistic(Mean) / (Std) of row[0..n) through an accessor (util.cpp:22-75: sequential float accumulation)
template <class F> __device__ __forceinline__ float seq_mean_f(const int n, F at) {
    float total = 0; int count = 0;
    for(int i = 0; i < n; ++i) { const float v = at(i); if(dev_valid(v)) { total += v; count++; } }
    return count > 0 ? total / (float)count : NAN;
}
template <class F> __device__ __forceinline__ float seq_std_f(const int n, F at) {
    float total = 0, total2 = 0, K = NAN; int count = 0;
    for(int i = 0; i < n; ++i) { const float v = at(i); if(dev_valid(v)) { if(!dev_valid(K)) K = v; const float d = v - K; total += d; total2 += d * d; count++; } }
    if(count == 0) return NAN;
    const float mean = total / (float)count, mean2 = total2 / (float)count;
    float var = mean2 - mean * mean;
    if(var < 0) var = 0;
    return sqrtf(var);
}

// per-observation ensemble quantities (oi_ensi_multi.cpp:421-444, :969-1003): one thread per observation
__global__ void k_multi_obs_prep(const int variant, const float* __restrict__ pbg, const float* __restrict__ pbgc, const float* __restrict__ pobs, int S, int E,
                                 const int* __restrict__ validIdx, int nV, float* __restrict__ gZ, float* __restrict__ gYm, float* __restrict__ gYhat,
                                 float* __restrict__ obs0) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if(s >= S) return;
    obs0[s] = variant == 3 ? pobs[s] : pobs[(long)s * E];
    gYhat[s] = 0.0f;
    if(variant == 3) {
        const float* row = pbg + (long)s * E;
        const float mean = seq_mean_f(nV, [&](int k) { return row[validIdx[k]]; });
        for(int k = 0; k < nV; ++k) gYm[(long)s * nV + k] = dev_valid(mean) ? row[validIdx[k]] - mean : 0.0f;
        gYhat[s] = mean;
    }
    if(variant != 2) {
        const float* row = pbgc + (long)s * E;
        const float mean = seq_mean_f(nV, [&](int k) { return row[validIdx[k]]; });
        const float sd = seq_std_f(nV, [&](int k) { return row[validIdx[k]]; });
        const bool ok = dev_valid(mean) && dev_valid(sd) && sd > 0.0013f;
        const float const_fact = (float)(1.0 / sqrt((double)(nV - 1)));
        for(int k = 0; k < nV; ++k) {
            float z = 0.0f;
            if(ok) {
                const float d = row[validIdx[k]] - mean;
                z = variant == 1 ? (float)(1.0 / sqrt((double)(nV - 1)) * (double)d / (double)sd) : (const_fact * d) / sd;
            }
            gZ[(long)s * nV + k] = z;
        }
    }
}
__global__ void k_iota(int* p, int n) { const int i = blockIdx.x * blockDim.x + threadIdx.x; if(i < n) p[i] = i; }

#define MULTI_N 64     // most selected observations of ebe / ebesc (LU in LDS)
template <int VARIANT>
__global__ __launch_bounds__(256) void k_ensi_multi(MultiArgs ma) {
    const EnsiArgs& a = ma.e;
    __shared__ double s_area[2 * 64 * EP];
    unsigned long long* const s_key = reinterpret_cast<unsigned long long*>(s_area);   // [EBIG_CAND]
    double* const s_B = s_area;
    double* const s_V = s_area + 64 * EP;
    __shared__ double s_t[64], s_w[64], s_X[64], s_cs[32], s_sn[32];
    __shared__ int s_p[32], s_q[32];
    __shared__ double s_off[256];
    __shared__ int s_n, s_piv;
    const int tid = threadIdx.x;
    const ScanArgs& sa = a.s;
    const DevStructure& st = sa.st;
    const int nV = a.nV, E = a.E;
    unsigned long long* const gkeys = a.big_keys + (size_t)blockIdx.x * EBIG_CAND;
    for(int cell = blockIdx.x; cell < a.C; cell += gridDim.x) {
        const float gx = a.gx[cell], gy = a.gy[cell], gz = a.gz[cell], ge = a.gelev[cell], gl = a.glaf[cell];
        __syncthreads();
        if(tid == 0) s_n = 0;
        __syncthreads();
        // ---- radius query + filter (valid observation, rho > 0: oi_ensi_multi.cpp:459-486) -----------------------------------------
        const float R = st.R;
        const float pa = sa.axis_a == 0 ? gx : (sa.axis_a == 1 ? gy : gz), pb = sa.axis_b == 1 ? gy : (sa.axis_b == 2 ? gz : gx);
        const int bx0 = min(max((int)floorf((pa - R - sa.amin) * sa.inv_s) - 1, 0), sa.nbx - 1), bx1 = min(max((int)floorf((pa + R - sa.amin) * sa.inv_s) + 1, 0), sa.nbx - 1);
        const int by0 = min(max((int)floorf((pb - R - sa.bmin) * sa.inv_s) - 1, 0), sa.nby - 1), by1 = min(max((int)floorf((pb + R - sa.bmin) * sa.inv_s) + 1, 0), sa.nby - 1);
        const float lox = gx - R, hix = gx + R, loy = gy - R, hiy = gy + R, loz = gz - R, hiz = gz + R;
        for(int by = by0; by <= by1; ++by) {
            const int js = sa.bin_start[by * sa.nbx + bx0], je = sa.bin_start[by * sa.nbx + bx1 + 1];
            for(int j = js + tid; j < je; j += 256) {
                const float4 rec = sa.pgeo[j];   // x = NaN for an unusable observation: fails the box test
                if(!(rec.x > lox && rec.x < hix && rec.y > loy && rec.y < hiy && rec.z > loz && rec.z < hiz)) continue;
                const float2 met = sa.smeta[j];
                if(!(d_chord(rec.x, rec.y, rec.z, gx, gy, gz) <= R)) continue;
                const float rho = d_corr(st, gx, gy, gz, ge, gl, rec.x, rec.y, rec.z, rec.w, met.x, true);
                if(!(rho > 0.0f)) continue;
                const int k = atomicAdd(&s_n, 1);
                if(k < EBIG_CAND) s_key[k] = ((unsigned long long)__float_as_uint(rho) << 32) | (unsigned)(~__float_as_int(met.y));
            }
        }
        __syncthreads();
        const int ncand = s_n;
        if(ncand == 0) continue;
        const bool truncated = sa.max_points > 0 && ncand > sa.max_points;
        const int n = truncated ? sa.max_points : ncand;
        if(ncand > EBIG_CAND || (VARIANT != 3 && n > MULTI_N)) {   // beyond the LDS areas of this kernel: k_ensi_multi_huge takes the cell
            if(tid == 0) a.huge_list[atomicAdd(a.big_count + 1, 1)] = cell;
            continue;
        }
        if(ma.oob) { if(tid == 0) atomicOr(a.err, 4); continue; }
        // ---- order: rho descending (ties -> lower index) when the reference sorts, index order otherwise; the max_points largest
        //      keys are picked by a radix select first (oi_common.h) and only they are sorted ---------------------------------------
        int nsort = ncand;
        if(truncated) { block_select_largest(s_key, ncand, n, gkeys, reinterpret_cast<int*>(s_off), &s_n, tid); nsort = n; }
        int np2 = 1;
        while(np2 < nsort) np2 <<= 1;
        for(int i = nsort + tid; i < np2; i += 256) s_key[i] = 0ull;
        __syncthreads();
        for(int k = 2; k <= np2; k <<= 1) {
            for(int j = k >> 1; j > 0; j >>= 1) {
                for(int i = tid; i < np2; i += 256) {
                    const int ixj = i ^ j;
                    if(ixj > i) {
                        const unsigned long long x = s_key[i], y = s_key[ixj];
                        const unsigned long long kx = truncated ? x : (x & 0xffffffffull), ky = truncated ? y : (y & 0xffffffffull);
                        const bool desc = (i & k) == 0;
                        if(desc ? (kx < ky) : (kx > ky)) { s_key[i] = y; s_key[ixj] = x; }
                    }
                }
                __syncthreads();
            }
        }
        for(int i = tid; i < n; i += 256) gkeys[i] = s_key[i];
        __threadfence_block();
        __syncthreads();
        const float ratio = ma.bratios[cell];
        if(VARIANT != 3) {
            // ---- K = r (A + R_dd)^-1: the transposed system in LDS, right-hand side in column n --------------------------------------------
            double* const A = s_area;                    // [n][MULTI_N + 1]
            const int AP = MULTI_N + 1;
            double* const xL = s_area + MULTI_N * AP;    // ebe: normalised perturbations of background_corr at this point [nV] (nV <= 4096)
            if(VARIANT == 1) {
                const float* rowc = ma.bgc + (long)cell * E;
                __shared__ float s_ms[2];
                if(tid == 0) {
                    s_ms[0] = seq_mean_f(nV, [&](int k) { return rowc[a.validIdx[k]]; });
                    s_ms[1] = seq_std_f(nV, [&](int k) { return rowc[a.validIdx[k]]; });
                }
                __syncthreads();
                const float mean = s_ms[0], sd = s_ms[1];
                const bool ok = dev_valid(mean) && dev_valid(sd) && sd > 0.0013f;
                for(int k = tid; k < nV; k += 256) xL[k] = ok ? 1.0 / sqrt((double)(nV - 1)) * (double)(rowc[a.validIdx[k]] - mean) / (double)sd : 0.0;   // :531-541
                __syncthreads();
            }
            for(int e2 = tid; e2 < n * n; e2 += 256) {
                const int i = e2 / n, j = e2 - i * n;
                const unsigned oi = ~(unsigned)(gkeys[i] & 0xffffffffull), oj = ~(unsigned)(gkeys[j] & 0xffffffffull);
                const float4 gi = a.ogeo[oi], gj = a.ogeo[oj];
                const float4 xi = a.oaux[oi], xj = a.oaux[oj];
                const float cc = d_corr(st, gi.x, gi.y, gi.z, gi.w, xi.x, gj.x, gj.y, gj.z, gj.w, xj.x, false);   // structure.corr(p_i, p_j), :570-577
                double zz = 1.0;
                if(VARIANT == 1) { zz = 0.0; for(int k = 0; k < nV; ++k) zz += (double)a.gY[(long)oi * nV + k] * (double)a.gY[(long)oj * nV + k]; }
                A[j * AP + i] = (double)cc * zz + (i == j ? (double)xi.w : 0.0);   // transposed: row j, column i
            }
            for(int i = tid; i < n; i += 256) {
                const unsigned long long key = gkeys[i];
                const unsigned oi = ~(unsigned)(key & 0xffffffffull);
                const float rho = __uint_as_float((unsigned)(key >> 32));
                double rz = 1.0;
                if(VARIANT == 1) { rz = 0.0; for(int k = 0; k < nV; ++k) rz += xL[k] * (double)a.gY[(long)oi * nV + k]; }
                A[i * AP + n] = (double)rho * rz;                                  // :581 / lCorr1D
            }
            __syncthreads();
            // pivoted LU (Gauss elimination with the right-hand side riding along)
            bool singular = false;
            for(int k = 0; k < n; ++k) {
                if(tid == 0) {
                    int p = k; double best = fabs(A[k * AP + k]);
                    for(int r = k + 1; r < n; ++r) { const double v = fabs(A[r * AP + k]); if(v > best) { best = v; p = r; } }
                    s_piv = (best > 0.0 && best < INFINITY) ? p : -1;
                }
                __syncthreads();
                const int p = s_piv;
                if(p < 0) { singular = true; break; }
                if(p != k) for(int cidx = tid; cidx <= n; cidx += 256) { const double t = A[k * AP + cidx]; A[k * AP + cidx] = A[p * AP + cidx]; A[p * AP + cidx] = t; }
                __syncthreads();
                const double pinv = 1.0 / A[k * AP + k];
                for(int e2 = tid; e2 < (n - k - 1) * (n - k); e2 += 256) {
                    const int r = k + 1 + e2 / (n - k), cidx = k + 1 + e2 % (n - k);
                    A[r * AP + cidx] -= A[r * AP + k] * pinv * A[k * AP + cidx];
                }
                __syncthreads();
            }
            if(singular) { if(tid == 0) atomicOr(a.err, 2); continue; }
            if(tid == 0) {   // back substitution: K in column n
                for(int r = n - 1; r >= 0; --r) {
                    double sacc = A[r * AP + n];
                    for(int cidx = r + 1; cidx < n; ++cidx) sacc -= A[r * AP + cidx] * A[cidx * AP + n];
                    A[r * AP + n] = sacc / A[r * AP + r];
                }
            }
            __syncthreads();
            // dx_e = ratio * K innov_e (:588), clamp (:593-615), out = background + dx (:620)
            for(int k = tid; k < nV; k += 256) {
                const int ei = a.validIdx[k];
                double sacc = 0.0; float maxInc = 0, minInc = 0;
                for(int i = 0; i < n; ++i) {
                    const unsigned oi = ~(unsigned)(gkeys[i] & 0xffffffffull);
                    const float inn = ma.pobs2[(long)oi * E + ei] - ma.pbg2[(long)oi * E + ei];
                    sacc = __builtin_fma(A[i * AP + n], (double)inn, sacc);
                    if(i == 0 || inn > maxInc) maxInc = inn;
                    if(i == 0 || inn < minInc) minInc = inn;
                }
                double dx = (double)ratio * sacc;
                if(!a.allow_extrap) {
                    float increment = (float)dx;
                    if(maxInc > 0 && increment > maxInc) increment = maxInc;
                    else if(maxInc < 0 && increment > 0) increment = 0;
                    else if(minInc < 0 && increment < minInc) increment = minInc;
                    else if(minInc > 0 && increment < 0) increment = 0;
                    dx = (double)increment;
                }
                a.out[(long)cell * E + ei] = (float)((double)a.bg[(long)cell * E + ei] + dx);
            }
            continue;
        }
        // ================================ utem: E x E square-root filter (:1060-1265) ==================================================
        float* const yc = reinterpret_cast<float*>(s_key);          // [64][64] Yc chunk
        double* const rinv = reinterpret_cast<double*>(yc + 64 * 64);
        double* const dvec = rinv + 64;
        double accP[16];
#pragma unroll
        for(int r = 0; r < 16; ++r) accP[r] = 0.0;
        double acct = 0.0;
        for(int i0 = 0; i0 < n; i0 += 64) {
            const int m = min(64, n - i0);
            __syncthreads();
            for(int e2 = tid; e2 < m * 64; e2 += 256) {
                const int i = e2 >> 6, k = e2 & 63;
                const unsigned orig = ~(unsigned)(gkeys[i0 + i] & 0xffffffffull);
                yc[i * 64 + k] = (k < nV) ? a.gY[(long)orig * nV + k] : 0.0f;
            }
            if(tid < m) {
                const unsigned long long key = gkeys[i0 + tid];
                const unsigned orig = ~(unsigned)(key & 0xffffffffull);
                const float4 x4 = a.oaux[orig];                       // laf, obs, gYhat, pratio
                rinv[tid] = (double)__uint_as_float((unsigned)(key >> 32)) / (double)x4.w;   // :1078
                dvec[tid] = (double)x4.y - (double)x4.z;
            }
            __syncthreads();
            for(int r = 0; r < 16; ++r) {
                const int e2 = tid + 256 * r, ai = e2 >> 6, bi = e2 & 63;
                if(ai < nV && bi < nV) {
                    double sacc = accP[r];
                    for(int i = 0; i < m; ++i) sacc = __builtin_fma((double)yc[i * 64 + ai] * rinv[i], (double)yc[i * 64 + bi], sacc);
                    accP[r] = sacc;
                }
            }
            if(tid < nV) for(int i = 0; i < m; ++i) acct = __builtin_fma((double)yc[i * 64 + tid] * rinv[i], dvec[i], acct);
        }
        __syncthreads();
        for(int r = 0; r < 16; ++r) {
            const int e2 = tid + 256 * r, ai = e2 >> 6, bi = e2 & 63;
            if(ai < nV && bi < nV) {
                s_B[ai * EP + bi] = accP[r] + (ai == bi ? 1.0 : 0.0);   // Pinv = C Yc + I (:1085)
                s_V[ai * EP + bi] = ai == bi ? 1.0 : 0.0;
            }
        }
        if(tid < nV) s_t[tid] = acct;
        __syncthreads();
        // cyclic Jacobi on the nV x nV matrix (as k_ensi_big)
        const int mm = nV + (nV & 1), half = mm >> 1;
        for(int sweep = 0; sweep < 40 && nV > 1; ++sweep) {
            double off2 = 0.0;
            // (scaled measure, see k_ensi_huge in ensi.hip)
            for(int e2 = tid; e2 < nV * nV; e2 += 256) { const int i = e2 / nV, j = e2 - i * nV; if(j < i) { const double vv = s_B[i * EP + j]; off2 += vv * vv / fmax(fabs(s_B[i * EP + i] * s_B[j * EP + j]), 1e-300); } }
            s_off[tid] = off2;
            __syncthreads();
            for(int off = 128; off > 0; off >>= 1) { if(tid < off) s_off[tid] += s_off[tid + off]; __syncthreads(); }
            off2 = s_off[0];
            __syncthreads();
            if(!(off2 > 1e-26)) break;
            for(int step = 0; step < mm - 1; ++step) {
                if(tid < half) {
                    int p, q;
                    if(tid == 0) { p = mm - 1; q = step; }
                    else { p = (step + tid) % (mm - 1); q = (step - tid + (mm - 1)) % (mm - 1); }
                    if(p > q) { const int t_ = p; p = q; q = t_; }
                    double cs = 1.0, sn = 0.0;
                    if(q < nV) {
                        const double apq = s_B[p * EP + q];
                        if(apq != 0.0) {
                            const double theta = (s_B[q * EP + q] - s_B[p * EP + p]) / (2.0 * apq);
                            const double t_ = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                            cs = 1.0 / sqrt(t_ * t_ + 1.0); sn = t_ * cs;
                            if(!(fabs(theta) < 1e150)) { cs = 1.0; sn = 0.0; }
                        }
                    }
                    else q = p;
                    s_p[tid] = p; s_q[tid] = q; s_cs[tid] = cs; s_sn[tid] = sn;
                }
                __syncthreads();
                const int pk = tid >> 3;
                const bool work = pk < half && s_p[pk] != s_q[pk];
                const int p = work ? s_p[pk] : 0, q = work ? s_q[pk] : 0;
                const double cs = work ? s_cs[pk] : 1.0, sn = work ? s_sn[pk] : 0.0;
                if(work)
                    for(int r = tid & 7; r < nV; r += 8) {
                        const double bp = s_B[r * EP + p], bq = s_B[r * EP + q];
                        const double vp = s_V[r * EP + p], vq = s_V[r * EP + q];
                        s_B[r * EP + p] = cs * bp - sn * bq; s_B[r * EP + q] = sn * bp + cs * bq;
                        s_V[r * EP + p] = cs * vp - sn * vq; s_V[r * EP + q] = sn * vp + cs * vq;
                    }
                __syncthreads();
                if(work)
                    for(int cidx = tid & 7; cidx < nV; cidx += 8) {
                        const double bp = s_B[p * EP + cidx], bq = s_B[q * EP + cidx];
                        s_B[p * EP + cidx] = cs * bp - sn * bq; s_B[q * EP + cidx] = sn * bp + cs * bq;
                    }
                __syncthreads();
            }
        }
        bool singular = false;
        if(tid < nV) { const double dk = s_B[tid * EP + tid]; singular = !(dk > 0.0) || isinf(dk); }
        s_off[tid] = singular ? 1.0 : 0.0;
        __syncthreads();
        for(int off = 128; off > 0; off >>= 1) { if(tid < off) s_off[tid] += s_off[tid + off]; __syncthreads(); }
        const bool skip = s_off[0] > 0.0;
        __syncthreads();
        if(skip) continue;   // rcond <= 0 -> raw values (:1087-1090)
        const double cscale = (double)(nV - 1);
        if(tid < nV) {
            double u = 0.0;
            for(int k = 0; k < nV; ++k) u = __builtin_fma(s_V[k * EP + tid], s_t[k], u);
            s_off[tid] = sqrt(cscale / s_B[tid * EP + tid]);        // eigenvalues of (nV - 1) P, square root (:1098-1121)
            s_X[tid] = u / s_B[tid * EP + tid];
        }
        __syncthreads();
        if(tid < nV) {
            double wv = 0.0;
            for(int k = 0; k < nV; ++k) wv = __builtin_fma(s_V[tid * EP + k], s_X[k], wv);
            s_w[tid] = wv;                                           // w = P C (lObs - lYhat)
        }
        __syncthreads();
        // ensemble statistics of this grid point (:1141-1179)
        __shared__ float s_val[64], s_valc[64], s_st[4];
        const int ek = (tid < nV) ? a.validIdx[tid] : 0;
        if(tid < nV) { s_val[tid] = a.bg[(long)cell * E + ek]; s_valc[tid] = ma.bgc[(long)cell * E + ek]; }
        __syncthreads();
        if(tid == 0) {
            float total = 0, totalc = 0;
            for(int k = 0; k < nV; ++k) { total += s_val[k]; totalc += s_valc[k]; }
            s_st[0] = total / (float)nV; s_st[2] = totalc / (float)nV;
            s_st[1] = seq_std_f(nV, [&](int k) { return s_val[k]; });
            s_st[3] = seq_std_f(nV, [&](int k) { return s_valc[k]; });
        }
        __syncthreads();
        const float ensMean = s_st[0], ensStd = s_st[1], ensMeanC = s_st[2], ensStdC = s_st[3];
        const float const_fact = (float)(1.0 / sqrt((double)(nV - 1)));
        for(int e2 = tid; e2 < nV * nV; e2 += 256) {
            const int ai = e2 / nV, bi = e2 - ai * nV;
            double sacc = 0.0;
            for(int k = 0; k < nV; ++k) sacc = __builtin_fma(s_V[ai * EP + k] * s_off[k], s_V[bi * EP + k], sacc);
            s_B[ai * EP + bi] = (double)ensStd * sacc + (double)ratio * s_w[ai];    // :1181-1185
        }
        __syncthreads();
        if(tid < nV) s_X[tid] = (ensStdC <= 0.0013f) ? 0.0 : (double)((const_fact * (s_valc[tid] - ensMeanC)) / ensStdC);   // X_corr
        __syncthreads();
        if(tid < nV) {
            float acc = 0.0f;
            for(int k = 0; k < nV; ++k) acc = (float)((double)acc + s_X[k] * s_B[k * EP + tid]);   // :1229-1233
            float currIncrement = acc;
            const double Xe = (double)s_val[tid] - (double)ensMean;
            if(!a.allow_extrap) {   // :1238-1262; lY[e] is a LINEAR index into the n x nV column-major matrix of the mean-removed pbackground
                const int li_ = tid % n, lk_ = tid / n;
                const unsigned oo = ~(unsigned)(gkeys[li_] & 0xffffffffull);
                const double lYe = (double)ma.gYm[(long)oo * nV + lk_];
                float maxInc = 0, minInc = 0;
                for(int i = 0; i < n; ++i) {
                    const unsigned oi_ = ~(unsigned)(gkeys[i] & 0xffffffffull);
                    const float4 x4 = a.oaux[oi_];
                    const float dv = (float)((double)x4.y - (lYe + (double)x4.z));
                    if(i == 0 || dv > maxInc) maxInc = dv;
                    if(i == 0 || dv < minInc) minInc = dv;
                }
                const float memberIncrement = (float)((double)currIncrement - Xe);
                if(maxInc > 0 && memberIncrement > maxInc) currIncrement = (float)((double)maxInc + Xe);
                else if(maxInc < 0 && memberIncrement > 0) currIncrement = (float)(0.0 + Xe);
                else if(minInc < 0 && memberIncrement < minInc) currIncrement = (float)((double)minInc + Xe);
                else if(minInc > 0 && memberIncrement < 0) currIncrement = (float)(0.0 + Xe);
            }
            a.out[(long)cell * E + ek] = ensMean + currIncrement;
        }
        __syncthreads();
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// k_ensi_multi_huge: the same three filters for the grid points k_ensi_multi cannot hold (more than MULTI_N selected
// observations for ebe / ebesc, more than EBIG_CAND candidates, more than 64 valid members for utem) -- the reference has
// no such limits (oi_ensi_multi.cpp:395-418, 489-505).  Keys, matrices and vectors live in HBM scratch sized by the host for
// the call (a.huge_keys, a.huge_mat); bitonic sort over global memory, pivoted LU / Jacobi in HBM.  Slow and general.
template <int VARIANT>
__global__ __launch_bounds__(256) void k_ensi_multi_huge(MultiArgs ma, const int* __restrict__ list, const int* __restrict__ count) {
    const EnsiArgs& a = ma.e;
    __shared__ float s_yc[16384];
    __shared__ double s_rinv[64], s_dvec[64];
    __shared__ double s_cs[32], s_sn[32];
    __shared__ int s_p[32], s_q[32];
    __shared__ double s_off[256];
    __shared__ float s_st[4];
    __shared__ int s_n, s_piv;
    const int tid = threadIdx.x;
    const ScanArgs& sa = a.s;
    const DevStructure& st = sa.st;
    const int nV = a.nV, E = a.E;
    const int nlist = count ? *count : a.C;
    unsigned long long* const keys = a.huge_keys + (size_t)blockIdx.x * a.huge_kcap;
    double* const scratch = a.huge_mat + (size_t)blockIdx.x * ma.huge_stride;
    auto block_sum = [&](double v) {
        s_off[tid] = v;
        __syncthreads();
        for(int off = 128; off > 0; off >>= 1) { if(tid < off) s_off[tid] += s_off[tid + off]; __syncthreads(); }
        const double r = s_off[0];
        __syncthreads();
        return r;
    };
    for(int li = blockIdx.x; li < nlist; li += gridDim.x) {
        const int cell = list ? list[li] : li;
        const float gx = a.gx[cell], gy = a.gy[cell], gz = a.gz[cell], ge = a.gelev[cell], gl = a.glaf[cell];
        __syncthreads();
        if(tid == 0) s_n = 0;
        __syncthreads();
        const float R = st.R;
        const float pa = sa.axis_a == 0 ? gx : (sa.axis_a == 1 ? gy : gz), pb = sa.axis_b == 1 ? gy : (sa.axis_b == 2 ? gz : gx);
        const int bx0 = min(max((int)floorf((pa - R - sa.amin) * sa.inv_s) - 1, 0), sa.nbx - 1), bx1 = min(max((int)floorf((pa + R - sa.amin) * sa.inv_s) + 1, 0), sa.nbx - 1);
        const int by0 = min(max((int)floorf((pb - R - sa.bmin) * sa.inv_s) - 1, 0), sa.nby - 1), by1 = min(max((int)floorf((pb + R - sa.bmin) * sa.inv_s) + 1, 0), sa.nby - 1);
        const float lox = gx - R, hix = gx + R, loy = gy - R, hiy = gy + R, loz = gz - R, hiz = gz + R;
        for(int by = by0; by <= by1; ++by) {
            const int js = sa.bin_start[by * sa.nbx + bx0], je = sa.bin_start[by * sa.nbx + bx1 + 1];
            for(int j = js + tid; j < je; j += 256) {
                const float4 rec = sa.pgeo[j];
                if(!(rec.x > lox && rec.x < hix && rec.y > loy && rec.y < hiy && rec.z > loz && rec.z < hiz)) continue;
                const float2 met = sa.smeta[j];
                if(!(d_chord(rec.x, rec.y, rec.z, gx, gy, gz) <= R)) continue;
                const float rho = d_corr(st, gx, gy, gz, ge, gl, rec.x, rec.y, rec.z, rec.w, met.x, true);
                if(!(rho > 0.0f)) continue;
                const int k = atomicAdd(&s_n, 1);
                if(k < a.huge_kcap) keys[k] = ((unsigned long long)__float_as_uint(rho) << 32) | (unsigned)(~__float_as_int(met.y));
            }
        }
        __syncthreads();
        const int ncand = s_n;
        if(ncand == 0) continue;
        const bool truncated = sa.max_points > 0 && ncand > sa.max_points;
        const int n = truncated ? sa.max_points : ncand;
        int np2 = 1;
        while(np2 < ncand) np2 <<= 1;
        if(np2 > a.huge_kcap || (VARIANT != 3 && n > ma.huge_ncap)) { if(tid == 0) atomicOr(a.err, 1); continue; }   // (sized for the call: cannot happen)
        if(ma.oob) { if(tid == 0) atomicOr(a.err, 4); continue; }
        for(int i = ncand + tid; i < np2; i += 256) keys[i] = 0ull;
        __threadfence_block();
        __syncthreads();
        for(int k = 2; k <= np2; k <<= 1) {
            for(int j = k >> 1; j > 0; j >>= 1) {
                for(int i = tid; i < np2; i += 256) {
                    const int ixj = i ^ j;
                    if(ixj > i) {
                        const unsigned long long x = keys[i], y = keys[ixj];
                        const unsigned long long kx = truncated ? x : (x & 0xffffffffull), ky = truncated ? y : (y & 0xffffffffull);
                        const bool desc = (i & k) == 0;
                        if(desc ? (kx < ky) : (kx > ky)) { keys[i] = y; keys[ixj] = x; }
                    }
                }
                __threadfence_block();
                __syncthreads();
            }
        }
        const float ratio = ma.bratios[cell];
        if(VARIANT != 3) {
            // ---- K = r (A + R_dd)^-1: the transposed system in HBM, right-hand side in column n (oi_ensi_multi.cpp:570-588) -----------
            double* const A = scratch;                               // [n][n + 1]
            const int AP = n + 1;
            double* const xL = scratch + (size_t)ma.huge_ncap * (ma.huge_ncap + 1);   // [nV]
            if(VARIANT == 1) {
                const float* rowc = ma.bgc + (long)cell * E;
                if(tid == 0) {
                    s_st[0] = seq_mean_f(nV, [&](int k) { return rowc[a.validIdx[k]]; });
                    s_st[1] = seq_std_f(nV, [&](int k) { return rowc[a.validIdx[k]]; });
                }
                __syncthreads();
                const float mean = s_st[0], sd = s_st[1];
                const bool ok = dev_valid(mean) && dev_valid(sd) && sd > 0.0013f;
                for(int k = tid; k < nV; k += 256) xL[k] = ok ? 1.0 / sqrt((double)(nV - 1)) * (double)(rowc[a.validIdx[k]] - mean) / (double)sd : 0.0;   // :531-541
                __threadfence_block();
                __syncthreads();
            }
            for(long e2 = tid; e2 < (long)n * n; e2 += 256) {
                const int i = (int)(e2 / n), j = (int)(e2 - (long)i * n);
                const unsigned oi = ~(unsigned)(keys[i] & 0xffffffffull), oj = ~(unsigned)(keys[j] & 0xffffffffull);
                const float4 gi = a.ogeo[oi], gj = a.ogeo[oj];
                const float4 xi = a.oaux[oi], xj = a.oaux[oj];
                const float cc = d_corr(st, gi.x, gi.y, gi.z, gi.w, xi.x, gj.x, gj.y, gj.z, gj.w, xj.x, false);
                double zz = 1.0;
                if(VARIANT == 1) { zz = 0.0; for(int k = 0; k < nV; ++k) zz += (double)a.gY[(long)oi * nV + k] * (double)a.gY[(long)oj * nV + k]; }
                A[(size_t)j * AP + i] = (double)cc * zz + (i == j ? (double)xi.w : 0.0);
            }
            for(int i = tid; i < n; i += 256) {
                const unsigned long long key = keys[i];
                const unsigned oi = ~(unsigned)(key & 0xffffffffull);
                const float rho = __uint_as_float((unsigned)(key >> 32));
                double rz = 1.0;
                if(VARIANT == 1) { rz = 0.0; for(int k = 0; k < nV; ++k) rz += xL[k] * (double)a.gY[(long)oi * nV + k]; }
                A[(size_t)i * AP + n] = (double)rho * rz;
            }
            __threadfence_block();
            __syncthreads();
            bool singular = false;
            for(int k = 0; k < n; ++k) {
                // pivot search: every thread scans a share of the column, the workgroup reduces (value, then lowest row)
                double best = -1.0; int bp = -1;
                for(int r = k + tid; r < n; r += 256) { const double v = fabs(A[(size_t)r * AP + k]); if(v > best) { best = v; bp = r; } }
                s_off[tid] = best;
                __syncthreads();
                for(int off = 128; off > 0; off >>= 1) { if(tid < off) s_off[tid] = fmax(s_off[tid], s_off[tid + off]); __syncthreads(); }
                const double gbest = s_off[0];
                __syncthreads();
                if(tid == 0) s_piv = 0x7fffffff;
                __syncthreads();
                if(bp >= 0 && best == gbest) atomicMin(&s_piv, bp);     // the first row holding the largest magnitude, as a sequential search finds it
                __syncthreads();
                const int p = (gbest > 0.0 && gbest < INFINITY) ? s_piv : -1;
                if(p < 0) { singular = true; break; }
                if(p != k) for(int cidx = tid; cidx <= n; cidx += 256) { const double t = A[(size_t)k * AP + cidx]; A[(size_t)k * AP + cidx] = A[(size_t)p * AP + cidx]; A[(size_t)p * AP + cidx] = t; }
                __threadfence_block();
                __syncthreads();
                const double pinv = 1.0 / A[(size_t)k * AP + k];
                const long nn = (long)(n - k - 1) * (n - k);
                for(long e2 = tid; e2 < nn; e2 += 256) {
                    const int r = k + 1 + (int)(e2 / (n - k)), cidx = k + 1 + (int)(e2 % (n - k));
                    A[(size_t)r * AP + cidx] -= A[(size_t)r * AP + k] * pinv * A[(size_t)k * AP + cidx];
                }
                __threadfence_block();
                __syncthreads();
            }
            if(singular) { if(tid == 0) atomicOr(a.err, 2); continue; }
            if(tid == 0) {
                for(int r = n - 1; r >= 0; --r) {
                    double sacc = A[(size_t)r * AP + n];
                    for(int cidx = r + 1; cidx < n; ++cidx) sacc -= A[(size_t)r * AP + cidx] * A[(size_t)cidx * AP + n];
                    A[(size_t)r * AP + n] = sacc / A[(size_t)r * AP + r];
                }
            }
            __threadfence_block();
            __syncthreads();
            for(int k = tid; k < nV; k += 256) {
                const int ei = a.validIdx[k];
                double sacc = 0.0; float maxInc = 0, minInc = 0;
                for(int i = 0; i < n; ++i) {
                    const unsigned oi = ~(unsigned)(keys[i] & 0xffffffffull);
                    const float inn = ma.pobs2[(long)oi * E + ei] - ma.pbg2[(long)oi * E + ei];
                    sacc = __builtin_fma(A[(size_t)i * AP + n], (double)inn, sacc);
                    if(i == 0 || inn > maxInc) maxInc = inn;
                    if(i == 0 || inn < minInc) minInc = inn;
                }
                double dx = (double)ratio * sacc;
                if(!a.allow_extrap) {
                    float increment = (float)dx;
                    if(maxInc > 0 && increment > maxInc) increment = maxInc;
                    else if(maxInc < 0 && increment > 0) increment = 0;
                    else if(minInc < 0 && increment < minInc) increment = minInc;
                    else if(minInc > 0 && increment < 0) increment = 0;
                    dx = (double)increment;
                }
                a.out[(long)cell * E + ei] = (float)((double)a.bg[(long)cell * E + ei] + dx);
            }
            continue;
        }
        // ================================ utem: E x E square-root filter (:1060-1265), everything in HBM ================================
        double* const B = scratch;
        double* const V = B + (size_t)nV * nV;
        double* const v_t = V + (size_t)nV * nV;
        double* const v_w = v_t + nV;
        double* const v_X = v_w + nV;
        double* const v_sq = v_X + nV;
        double* const v_val = v_sq + nV;
        double* const v_valc = v_val + nV;
        const int chunk = max(1, min(64, 16384 / max(nV, 1)));
        for(long e = tid; e < (long)nV * nV; e += 256) { const int ai = (int)(e / nV), bi = (int)(e - (long)ai * nV); B[e] = 0.0; V[e] = (ai == bi) ? 1.0 : 0.0; }
        for(int k = tid; k < nV; k += 256) v_t[k] = 0.0;
        __threadfence_block();
        __syncthreads();
        for(int i0 = 0; i0 < n; i0 += chunk) {
            const int m = min(chunk, n - i0);
            for(int e = tid; e < m * nV; e += 256) {
                const int i = e / nV, k = e - i * nV;
                const unsigned orig = ~(unsigned)(keys[i0 + i] & 0xffffffffull);
                s_yc[i * nV + k] = a.gY[(long)orig * nV + k];
            }
            if(tid < m) {
                const unsigned long long key = keys[i0 + tid];
                const unsigned orig = ~(unsigned)(key & 0xffffffffull);
                const float4 x4 = a.oaux[orig];                       // laf, obs, gYhat, pratio
                s_rinv[tid] = (double)__uint_as_float((unsigned)(key >> 32)) / (double)x4.w;   // :1078
                s_dvec[tid] = (double)x4.y - (double)x4.z;
            }
            __syncthreads();
            for(long e = tid; e < (long)nV * nV; e += 256) {
                const int ai = (int)(e / nV), bi = (int)(e - (long)ai * nV);
                double sacc = B[e];
                for(int i = 0; i < m; ++i) sacc = __builtin_fma((double)s_yc[i * nV + ai] * s_rinv[i], (double)s_yc[i * nV + bi], sacc);
                B[e] = sacc;
            }
            for(int k = tid; k < nV; k += 256) {
                double acct = v_t[k];
                for(int i = 0; i < m; ++i) acct = __builtin_fma((double)s_yc[i * nV + k] * s_rinv[i], s_dvec[i], acct);
                v_t[k] = acct;
            }
            __threadfence_block();
            __syncthreads();
        }
        for(int k = tid; k < nV; k += 256) B[(size_t)k * nV + k] += 1.0;    // Pinv = C Yc + I (:1085)
        __threadfence_block();
        __syncthreads();
        const int mm = nV + (nV & 1), half = mm >> 1;
        for(int sweep = 0; sweep < 60 && nV > 1; ++sweep) {
            double off2 = 0.0;
            // (the products of diagonals floored at 1e-300: a zero or denormal diagonal must read as "not converged", not as 0 / 0 = NaN = stop)
            // Stopping test in the SCALED measure sum (b_ij^2 / |b_ii b_jj|) <= 1e-26 (Demmel / Veselic: every eigenvalue and eigenvector of a positive
            // definite matrix to high RELATIVE accuracy).  Until round 5 the test was |off|_F <= 1e-11 trace: with observation sigmas x 0.01 the
            // spectrum of Pinv spans c ... 1e7 and the eigenvectors of the SMALL eigenvalues -- the ones that carry the weight in sqrt(c / D) --
            // were left with errors of 1e-5 (36 % of the float32 outputs off by an ulp, 1.5e-4 in the plain measure; k_ensi_huge, ensi.hip)
            for(long e = tid; e < (long)nV * nV; e += 256) { const int i = (int)(e / nV), j = (int)(e - (long)i * nV); if(j < i) { const double v = B[e]; off2 += v * v / fmax(fabs(B[(size_t)i * nV + i] * B[(size_t)j * nV + j]), 1e-300); } }
            off2 = block_sum(off2);
            if(!(off2 > 1e-26)) break;   // (also on NaN: a non-finite matrix)
            for(int step = 0; step < mm - 1; ++step) {
                for(int g0 = 0; g0 < half; g0 += 32) {
                    const int npair = min(32, half - g0);
                    if(tid < npair) {
                        const int t = g0 + tid;
                        int p, q;
                        if(t == 0) { p = mm - 1; q = step; }
                        else { p = (step + t) % (mm - 1); q = (step - t + (mm - 1)) % (mm - 1); }
                        if(p > q) { const int t_ = p; p = q; q = t_; }
                        double cs = 1.0, sn = 0.0;
                        if(q < nV) {
                            const double apq = B[(size_t)p * nV + q];
                            if(apq != 0.0) {
                                const double theta = (B[(size_t)q * nV + q] - B[(size_t)p * nV + p]) / (2.0 * apq);
                                const double t_ = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                                cs = 1.0 / sqrt(t_ * t_ + 1.0); sn = t_ * cs;
                                if(!(fabs(theta) < 1e150)) { cs = 1.0; sn = 0.0; }
                            }
                        }
                        else q = p;
                        s_p[tid] = p; s_q[tid] = q; s_cs[tid] = cs; s_sn[tid] = sn;
                    }
                    __syncthreads();
                    const int pk = tid >> 3;
                    const bool work = pk < npair && s_p[pk] != s_q[pk];
                    const int p = work ? s_p[pk] : 0, q = work ? s_q[pk] : 0;
                    const double cs = work ? s_cs[pk] : 1.0, sn = work ? s_sn[pk] : 0.0;
                    if(work)
                        for(int r = tid & 7; r < nV; r += 8) {
                            const double bp = B[(size_t)r * nV + p], bq = B[(size_t)r * nV + q];
                            const double vp = V[(size_t)r * nV + p], vq = V[(size_t)r * nV + q];
                            B[(size_t)r * nV + p] = cs * bp - sn * bq; B[(size_t)r * nV + q] = sn * bp + cs * bq;
                            V[(size_t)r * nV + p] = cs * vp - sn * vq; V[(size_t)r * nV + q] = sn * vp + cs * vq;
                        }
                    __threadfence_block();
                    __syncthreads();
                    if(work)
                        for(int cidx = tid & 7; cidx < nV; cidx += 8) {
                            const double bp = B[(size_t)p * nV + cidx], bq = B[(size_t)q * nV + cidx];
                            B[(size_t)p * nV + cidx] = cs * bp - sn * bq; B[(size_t)q * nV + cidx] = sn * bp + cs * bq;
                        }
                    __threadfence_block();
                    __syncthreads();
                }
            }
        }
        double bad = 0.0;
        for(int k = tid; k < nV; k += 256) { const double dk = B[(size_t)k * nV + k]; if(!(dk > 0.0) || isinf(dk)) bad = 1.0; }
        if(block_sum(bad) > 0.0) continue;   // rcond <= 0 -> raw values (:1087-1090)
        const double cscale = (double)(nV - 1);
        for(int k = tid; k < nV; k += 256) {
            double u = 0.0;
            for(int r = 0; r < nV; ++r) u = __builtin_fma(V[(size_t)r * nV + k], v_t[r], u);
            v_sq[k] = sqrt(cscale / B[(size_t)k * nV + k]);
            v_X[k] = u / B[(size_t)k * nV + k];
        }
        __threadfence_block();
        __syncthreads();
        for(int k = tid; k < nV; k += 256) {
            double wv = 0.0;
            for(int r = 0; r < nV; ++r) wv = __builtin_fma(V[(size_t)k * nV + r], v_X[r], wv);
            v_w[k] = wv;
        }
        for(int k = tid; k < nV; k += 256) { const int ek = a.validIdx[k]; v_val[k] = (double)a.bg[(long)cell * E + ek]; v_valc[k] = (double)ma.bgc[(long)cell * E + ek]; }
        __threadfence_block();
        __syncthreads();
        if(tid == 0) {   // ensemble statistics of this grid point (:1141-1179)
            float total = 0, totalc = 0;
            for(int k = 0; k < nV; ++k) { total += (float)v_val[k]; totalc += (float)v_valc[k]; }
            s_st[0] = total / (float)nV; s_st[2] = totalc / (float)nV;
            s_st[1] = seq_std_f(nV, [&](int k) { return (float)v_val[k]; });
            s_st[3] = seq_std_f(nV, [&](int k) { return (float)v_valc[k]; });
        }
        __syncthreads();
        const float ensMean = s_st[0], ensStd = s_st[1], ensMeanC = s_st[2], ensStdC = s_st[3];
        const float const_fact = (float)(1.0 / sqrt((double)(nV - 1)));
        for(long e = tid; e < (long)nV * nV; e += 256) {
            const int ai = (int)(e / nV), bi = (int)(e - (long)ai * nV);
            double sacc = 0.0;
            for(int k = 0; k < nV; ++k) sacc = __builtin_fma(V[(size_t)ai * nV + k] * v_sq[k], V[(size_t)bi * nV + k], sacc);
            B[e] = (double)ensStd * sacc + (double)ratio * v_w[ai];    // :1181-1185
        }
        for(int k = tid; k < nV; k += 256) v_X[k] = (ensStdC <= 0.0013f) ? 0.0 : (double)((const_fact * ((float)v_valc[k] - ensMeanC)) / ensStdC);   // X_corr
        __threadfence_block();
        __syncthreads();
        for(int e = tid; e < nV; e += 256) {
            float acc = 0.0f;
            for(int k = 0; k < nV; ++k) acc = (float)((double)acc + v_X[k] * B[(size_t)k * nV + e]);   // :1229-1233
            float currIncrement = acc;
            const double Xe = v_val[e] - (double)ensMean;
            if(!a.allow_extrap) {
                const int li_ = e % n, lk_ = e / n;
                const unsigned oo = ~(unsigned)(keys[li_] & 0xffffffffull);
                const double lYe = (double)ma.gYm[(long)oo * nV + lk_];
                float maxInc = 0, minInc = 0;
                for(int i = 0; i < n; ++i) {
                    const unsigned oi_ = ~(unsigned)(keys[i] & 0xffffffffull);
                    const float4 x4 = a.oaux[oi_];
                    const float dv = (float)((double)x4.y - (lYe + (double)x4.z));
                    if(i == 0 || dv > maxInc) maxInc = dv;
                    if(i == 0 || dv < minInc) minInc = dv;
                }
                const float memberIncrement = (float)((double)currIncrement - Xe);
                if(maxInc > 0 && memberIncrement > maxInc) currIncrement = (float)((double)maxInc + Xe);
                else if(maxInc < 0 && memberIncrement > 0) currIncrement = (float)(0.0 + Xe);
                else if(minInc < 0 && memberIncrement < minInc) currIncrement = (float)((double)minInc + Xe);
                else if(minInc > 0 && memberIncrement < 0) currIncrement = (float)(0.0 + Xe);
            }
            a.out[(long)cell * E + a.validIdx[e]] = ensMean + currIncrement;
        }
        __syncthreads();
    }
}
