// cr_cos.h -- cos(x) in float64, correctly rounded in all but a vanishing share of cases, host and device.
//
// The evaluator's orientation similarity (eval.py:264) is (1 + cos(delta)) / 2 per true positive: where cos(delta) is near -1
// the sum cancels and a last-bit difference of cos becomes several ulps of the term. numpy's cos (the C library's) is correctly
// rounded for practically every argument; the device library's is not. So the kernel evaluates cos in double-double (about 100
// bits: three-part Cody-Waite reduction by pi/2 with the constants of fdlibm's e_rem_pio2.c, then the Taylor series in nested
// form, every operation error-free or double-double) and rounds once. -ffp-contract=off keeps the error-free transformations
// intact; the products' low parts come from explicit fma().
#pragma once
#include <math.h>

#include "cr_trig.h"  // EPNET_HD

namespace epnet {

struct dd {
    double hi, lo;
};

EPNET_HD dd two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
EPNET_HD dd quick_two_sum(double a, double b) {  // |a| >= |b|
    const double s = a + b;
    return {s, b - (s - a)};
}
EPNET_HD dd two_prod(double a, double b) {
    const double p = a * b;
    return {p, fma(a, b, -p)};
}
EPNET_HD dd dd_add_d(dd a, double b) {
    dd s = two_sum(a.hi, b);
    s.lo += a.lo;
    return quick_two_sum(s.hi, s.lo);
}
EPNET_HD dd dd_mul(dd a, dd b) {
    dd p = two_prod(a.hi, b.hi);
    p.lo += a.hi * b.lo + a.lo * b.hi;
    return quick_two_sum(p.hi, p.lo);
}
EPNET_HD dd dd_div_d(dd a, double d) {
    const double q1 = a.hi / d;
    const double r = fma(-q1, d, a.hi) + a.lo;
    return quick_two_sum(q1, r / d);
}

EPNET_HD double cr_cos(double x) {
    if (!(fabs(x) < 1048576.0)) return cos(x);  // beyond the exact range of the reduction (and NaN / inf): the library's
    // pi/2 in 33 + 33 + 33 + 53 bits (fdlibm): k * each of the first three is exact for |k| < 2^20
    const double pio2_1 = 1.57079632673412561417e+00, pio2_2 = 6.07710050630396597660e-11, pio2_3 = 2.02226624871116645580e-21,
                 pio2_3t = 8.47842766036889956997e-32;
    const double k = rint(x * 6.36619772367581382433e-01);
    dd r = two_sum(x, -k * pio2_1);
    r = dd_add_d(r, -k * pio2_2);
    r = dd_add_d(r, -k * pio2_3);
    r = dd_add_d(r, -k * pio2_3t);
    const dd r2 = dd_mul(r, r);
    const int n = (int)k & 3;
    // |r| <= pi/4 (+ one ulp of the quotient): r^30 / 30! < 2^-118. cos: m = 1, 3, ..; sin: m = 2, 4, ..;
    // t <- 1 - r^2 t / (m (m + 1)), innermost term first
    dd t = {1.0, 0.0};
    for (int m = (n & 1) ? 30 : 29; m >= 1; m -= 2) {
        dd u = dd_div_d(dd_mul(r2, t), (double)(m * (m + 1)));
        u.hi = -u.hi;
        u.lo = -u.lo;
        t = dd_add_d(u, 1.0);
    }
    if (n & 1) t = dd_mul(r, t);  // sin r
    const double v = t.hi + t.lo;
    return (n == 1 || n == 2) ? -v : v;
}

}  // namespace epnet
