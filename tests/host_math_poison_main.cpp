// Stand-alone driver of tests/host_math_harness.cpp (the product's per-Gaussian math, csrc/gsr_math.h, built for the host) for a build under
// -fsanitize=undefined,float-cast-overflow: tests/test_poison_cpu.py writes frames with non-finite and out-of-range parameters to files, this
// program projects each of them with antialiasing off and on, snug and reference rectangles, the whole grid and a band of tile rows, and the
// sanitizer ends it at the first float that is converted to an integer it does not fit (a NaN tile coordinate, an infinite radius) or any other
// undefined operation.  File: HostCam, int32 P, int32 has_cov, int32 has_colors, then float32 means[P*3], scales[P*3], rotations[P*4], cov[P*6],
// opacities[P], shs[P*M*3], colors[P*3] (all present; the flags say which the call uses).  Prints the sum of tiles_touched per configuration.
// Test infrastructure: nothing in the package loads it.
#include <cstdio>
#include <vector>
#include "host_math_harness.cpp"

static bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        HostCam hc;
        int hdr[3];
        if (!f || !rd(f, &hc, sizeof(hc)) || !rd(f, hdr, sizeof(hdr))) { fprintf(stderr, "%s: cannot read\n", argv[a]); return 2; }
        const int P = hdr[0], M = hc.M;
        std::vector<float> means(P * 3), scales(P * 3), rots(P * 4), cov(P * 6), opac(P), shs((size_t)P * M * 3), colors(P * 3);
        for (std::vector<float>* v : {&means, &scales, &rots, &cov, &opac, &shs, &colors})
            if (!rd(f, v->data(), v->size() * sizeof(float))) { fprintf(stderr, "%s: short file\n", argv[a]); return 2; }
        fclose(f);
        std::vector<float> out_f(P * 12), out_cov(P * 6);
        std::vector<int> out_i(P * 8);
        for (int aa = 0; aa < 2; ++aa)
            for (int snug = 0; snug < 2; ++snug)
                for (int band = 0; band < 2; ++band) {
                    hc.antialiasing = aa;
                    hc.tile_y0 = band ? 2 : 0;
                    hc.tile_y1 = band ? 5 : 0;
                    host_set_snug(snug);
                    host_preprocess(&hc, P, means.data(), hdr[1] ? nullptr : scales.data(), hdr[1] ? nullptr : rots.data(), hdr[1] ? cov.data() : nullptr,
                                    opac.data(), hdr[2] ? nullptr : shs.data(), hdr[2] ? colors.data() : nullptr, out_f.data(), out_i.data(), out_cov.data());
                    long tiles = 0;
                    for (int i = 0; i < P; ++i) tiles += out_i[8 * i + 5];
                    printf("%s aa=%d snug=%d band=%d tiles=%ld\n", argv[a], aa, snug, band, tiles);
                }
    }
    return 0;
}
