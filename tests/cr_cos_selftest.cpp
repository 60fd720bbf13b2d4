// prints cr_cos (epnet_amd/csrc/cr_cos.h, the host build of the device function) of every argument given on the command line,
// as the 16 hex digits of the float64 result
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdint.h>

#include "cr_cos.h"

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        const double v = epnet::cr_cos(strtod(argv[i], nullptr));
        uint64_t bits;
        memcpy(&bits, &v, 8);
        printf("%016llx\n", (unsigned long long)bits);
    }
    return 0;
}
