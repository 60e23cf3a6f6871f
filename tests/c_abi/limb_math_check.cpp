// csrc/limb_math.h (and the two helpers it takes from csrc/shg_common.h) compiled by the host compiler: the limb stage's shared
// arithmetic evaluated on the CPU, for the test to put next to NumPy.
//   limb_math_check <what> <in> <out>     <in>: raw float64, <out>: raw 8-byte words
//     hypot   pairs (x, y)                 -> hypot_glibc(x, y)
//     lerp    triples (a, b, gamma)        -> np_lerp(a, b, gamma)
//     keys    values x                     -> per value: f64_key(x) (uint64), key_f64(f64_key(x))
//     refl    pairs (i, n)                 -> refl(i, n) as float64
//     hist    (mn, mx), then values        -> the 21 edges, then per value its bin as float64
#include <stdio.h>
#include <string.h>
#include <vector>
#include "limb_math.h"

using namespace shg::limb;

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 3;
    std::vector<double> in;
    double buf[1024];
    for (size_t got; (got = fread(buf, 8, 1024, f)) > 0;) in.insert(in.end(), buf, buf + got);
    fclose(f);
    std::vector<uint64_t> out;
    auto put = [&](double v) { uint64_t b; memcpy(&b, &v, 8); out.push_back(b); };
    const size_t n = in.size();
    if (!strcmp(argv[1], "hypot")) {
        for (size_t i = 0; i + 1 < n; i += 2) put(hypot_glibc(in[i], in[i + 1]));
    } else if (!strcmp(argv[1], "lerp")) {
        for (size_t i = 0; i + 2 < n; i += 3) put(shg::np_lerp(in[i], in[i + 1], in[i + 2]));
    } else if (!strcmp(argv[1], "keys")) {
        for (size_t i = 0; i < n; ++i) { out.push_back(shg::f64_key(in[i])); put(shg::key_f64(shg::f64_key(in[i]))); }
    } else if (!strcmp(argv[1], "refl")) {
        for (size_t i = 0; i + 1 < n; i += 2) put((double)refl((int)in[i], (int)in[i + 1]));
    } else if (!strcmp(argv[1], "hist")) {
        if (n < 2) return 4;
        double edges[HIST_BINS + 1];
        for (int i = 0; i <= HIST_BINS; ++i) put(edges[i] = hist_edge(in[0], in[1], i));
        for (size_t i = 2; i < n; ++i) put((double)hist_bin([&](int j) { return edges[j]; }, in[i]));
    } else {
        return 2;
    }
    f = fopen(argv[3], "wb");
    if (!f) return 3;
    const bool ok = fwrite(out.data(), 8, out.size(), f) == out.size();
    return fclose(f) == 0 && ok ? 0 : 5;
}
