// test helper: the host twin of the device split (csrc/ssal_bf16x3.h: ssal::bf16x3::split_host) on a file of fp32 values.
// usage: split_host_terms <in: n floats> <out: n x 3 uint32 terms>; built by tests/test_split_operand_model_cpu.py
#define __host__
#define __device__
#include "ssal_bf16x3.h"

#include <stdio.h>

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 3;
    float x;
    while (fread(&x, 4, 1, in) == 1) {
        uint32_t t[3];
        ssal::bf16x3::split_host(x, t);
        if (fwrite(t, 4, 3, out) != 3) return 4;
    }
    fclose(in);
    return fclose(out) ? 5 : 0;
}
