// test helper: the host packer of ICNet's bf16x3 kernel operand (csrc/ssal_bf16x3.h: ssal::bf16x3::pack_igemm) on a file.
// usage: icnet_split_pack <kh> <kw> <cin> <cout> <in: kh*kw*cin*cout floats, HWIO> <out: the packed units>; built by
// tests/test_icnet_bf16x3_cpu.py (plain and with the host sanitizers: the packer is host code)
#define __host__
#define __device__
#include "ssal_bf16x3.h"

#include <stdio.h>
#include <stdlib.h>

int main(int argc, char **argv)
{
    if (argc != 7) return 2;
    const int kh = atoi(argv[1]), kw = atoi(argv[2]), cin = atoi(argv[3]), cout = atoi(argv[4]);
    if (kh < 1 || kw < 1 || cin < 16 || cin % 16 || cout < 1) return 2;
    FILE *in = fopen(argv[5], "rb"), *out = fopen(argv[6], "wb");
    if (!in || !out) return 3;
    std::vector<float> w((size_t)kh * kw * cin * cout);
    if (fread(w.data(), 4, w.size(), in) != w.size()) return 4;
    const std::vector<float> p = ssal::bf16x3::pack_igemm(w.data(), kh, kw, cin, cout);
    if (p.size() != ssal::bf16x3::igemm_units(kh, kw, cin, cout) * 4) return 5;
    if (fwrite(p.data(), 4, p.size(), out) != p.size()) return 6;
    fclose(in);
    return fclose(out) ? 7 : 0;
}
