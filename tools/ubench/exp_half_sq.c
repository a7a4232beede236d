/* exp(-v^2 / 2) of d_barnes_rho_flat (gridpp_amd/csrc/oi_common.h) restated for the CPU in its two forms: d_exp_core(-0.5 v v), and
   d_exp_half_neg(v v) with the factor -1/2 folded into the constants.  Every scaling is by a power of two, so the two must return the very
   same double.  usage: exp_half_sq [stride]: every stride-th float32 v in [0, 15] by bit pattern, and v = 0, 15, the smallest normal, a
   subnormal and the largest subnormal; tests/test_exp_half_sq.py runs it. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
static const double T[128] = {
#include "exp_table_tab.inc"
};
static double e_core(double x){
    const double kf = rint(x * 184.66496523378730813);
    double r = fma(kf, -6.93147180369123816490e-01 / 128.0, x);
    r = fma(kf, -1.90821492927058770002e-10 / 128.0, r);
    const int k = (int)kf;
    const double t = T[k & 127];
    double p = 8.33333333333333333333e-03;
    p = fma(p, r, 4.16666666666666666667e-02);
    p = fma(p, r, 1.66666666666666666667e-01);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = p * r;
    p = fma(t, p, t);
    return ldexp(p, k >> 7);
}
static double e_half_neg(double t){
    const double kf = rint(t * (-184.66496523378730813 / 2.0));
    double r = fma(kf, 6.93147180369123816490e-01 / 64.0, t);
    r = fma(kf, 1.90821492927058770002e-10 / 64.0, r);
    const int k = (int)kf;
    const double tb = T[k & 127];
    double p = -8.33333333333333333333e-03 / 32.0;
    p = fma(p, r, 4.16666666666666666667e-02 / 16.0);
    p = fma(p, r, -1.66666666666666666667e-01 / 8.0);
    p = fma(p, r, 0.125);
    p = fma(p, r, -0.5);
    p = p * r;
    p = fma(tb, p, tb);
    return ldexp(p, k >> 7);
}
static long n = 0, bad = 0;
static void check(uint32_t bits){
    float v; memcpy(&v, &bits, 4);
    v = fminf(fabsf(v), 15.0f);
    const double a = e_core(-0.5 * (double)v * (double)v), b = e_half_neg((double)v * (double)v);
    n++;
    if(memcmp(&a, &b, 8) != 0){ if(bad++ < 10) printf("v=%a old=%a new=%a\n", (double)v, a, b); }
}
int main(int argc, char** argv){
    const uint32_t stride = argc > 1 ? (uint32_t)atol(argv[1]) : 64u, top = 0x41700000u;   /* 15.0f */
    for(uint32_t b = 0; b <= top - stride; b += stride) check(b);
    check(0u); check(top); check(0x00800000u); check(0x00000001u); check(0x00012345u); check(0x007fffffu);
    printf("n=%ld mismatches %ld\n", n, bad);
    return bad != 0;
}
