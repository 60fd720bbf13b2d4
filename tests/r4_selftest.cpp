// compares r4 (epnet_amd/csrc/r4.h, the host build of the device function) with snprintf("%.4f") + strtod, bit for bit, on: every
// half-unit tie (k + 0.5) / 1e4 that is exactly a float (the odd multiples of 1/32) up to 2^21 / 32 in both signs, small negative
// values that print as -0.0000, denormals, 1e30f, FLT_MAX, infinities, NaN, and a million pseudo-random bit patterns. Prints the
// number of values and of differences; the exit status is 0 only without a difference.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdint.h>

#include "r4.h"

static long checked = 0, differ = 0;

static void check(float v) {
    char text[128];
    snprintf(text, sizeof text, "%.4f", (double)v);
    const double want = strtod(text, nullptr), got = epnet::r4(v);
    ++checked;
    if (std::isnan(want) && std::isnan(got)) return;
    if (memcmp(&want, &got, 8) != 0) {
        if (++differ <= 10) fprintf(stderr, "r4(%.9g) = %.17g, the text \"%s\" parses to %.17g\n", (double)v, got, text, want);
    }
}

int main() {
    long ties = 0;
    for (long q = 1; q < (1L << 21); q += 2) {  // q / 32 * 1e4 = q * 312.5: a tie for every odd q
        const float v = (float)q / 32.0f;
        check(v);
        check(-v);
        ties += 2;
    }
    const float special[] = {0.0f, -0.0f, -1e-5f, -4.9e-5f, -5e-5f, -5.0001e-5f, 5e-5f, 1.5e-4f, 1e-45f, -1e-45f, 1e-39f, FLT_MIN,
                             1e30f, -1e30f, FLT_MAX, -FLT_MAX, INFINITY, -INFINITY, NAN, 0.12345f, 1241.0f, 3.14159274f};
    for (float v : special) check(v);
    uint32_t state = 12345u;
    for (int i = 0; i < 1000000; ++i) {  // every exponent, denormals, infinities and NaNs among them
        state = state * 1664525u + 1013904223u;
        float v;
        memcpy(&v, &state, 4);
        check(v);
        state = state * 1664525u + 1013904223u;  // and values of the size the records hold
        check((float)((int32_t)state) / 1048576.0f);
    }
    printf("%ld values (%ld ties), %ld differences\n", checked, ties, differ);
    return differ == 0 ? 0 : 1;
}
