// tools/check_yuv_fast_422.cpp — exhaustive proof that the PAIR chroma of the output conversion's fast path (packed 4:2:2 outputs:
// yuvfast::convert422<plane>() of smelter_amd/csrc/smr_yuv_fast.h, THE header the kernels include) never yields a byte that differs from the
// reference sequence (rgba_to_yuv.wgsl:26-54 as yuv_byte() / unorm_of_byte() restate it, with the 4:2:2 chroma sample a * .5 + b * .5 of a
// horizontal pixel pair) without raising its guard flag.  The twin of tools/check_yuv_fast.cpp, which proves luma (convert<0>, used unchanged
// by the packed store) and the 2x2 block chroma.
//
//   fast:   x = fma(R, k_r, fma(G, k_g, fma(B, k_b, k_0 + delta)))      (R, G, B: the pair's byte sums, 0 .. 510)
//           byte = trunc(x);   flag = fract(x) < 2 delta   ->  flagged values are recomputed with the reference sequence
//   exact:  the f32 sequence of the WGSL pass, operation by operation (compiled here with -ffp-contract=off)
//
// The pair chroma is a function of the three channels' means m = a/255 * .5 + b/255 * .5; m depends on the two bytes only through the f32
// values the expression takes for their sum.  The tool enumerates, per sum S in 0..510, the SET of values m takes over all ordered byte pairs,
// then checks every combination (S_r, S_g, S_b) x (every m_r, m_g, m_b of the sets): the complete domain.  It prints the largest deviation of
// the fast value from the sequence's value before truncation next to the guard band the kernels use, and the flagged share.
//
// build:  g++ -O2 -fopenmp -ffp-contract=off -I smelter_amd/csrc -o check_yuv_fast_422 tools/check_yuv_fast_422.cpp
// run:    check_yuv_fast_422          the complete domain (133 M sum triples per plane)
//         check_yuv_fast_422 quick    every 8th red sum (tests/test_yuv_fast_422.py)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "smr_yuv_fast.h"

#define GUARD (yuvfast::DELTA422)

static float unorm_of_byte(uint32_t b) {
    const float a = (float)b;
    return fmaf(a, 1.0f / 255.0f, a * -1.1641532182693481e-10f);
}
static uint32_t yuv_byte(float r, float g, float b, int plane, float *pre) {
    float comp;
    if (plane == 1) {
        const float u = r * -0.1146f + g * -0.3854f + b * 0.5f;
        comp = ((u + 0.5f) * 0.87843137254f) + (16.0f / 255.0f);
    } else {
        const float v = r * 0.5f + g * -0.4542f + b * -0.0458f;
        comp = ((v + 0.5f) * 0.87843137254f) + (16.0f / 255.0f);
    }
    const float t = comp * 255.0f + 0.5f;
    if (pre) *pre = t;
    return (uint32_t)(int)t;
}

static inline uint32_t fast_convert(int plane, float r, float g, float b, bool *flag) {
    return plane == 1 ? yuvfast::convert422<1>(r, g, b, flag) : yuvfast::convert422<2>(r, g, b, flag);
}
static inline float fast_x(int plane, float r, float g, float b) {  // the value convert422() truncates (for the deviation statistics only)
    const yuvfast::K k = yuvfast::constants422(plane);
    return fmaf(r, k.kr, fmaf(g, k.kg, fmaf(b, k.kb, k.k0)));
}

int main(int argc, char **argv) {
    const bool quick = argc > 1 && !strcmp(argv[1], "quick");
    int bad = 0;
    // ------------------------------------------------------------------ the sets of pair means per byte sum
    enum { NS = 511, MAXSET = 8 };
    static float set[NS][MAXSET];
    static int nset[NS];
    {
        float n[256];
        for (int i = 0; i < 256; i++) n[i] = unorm_of_byte((uint32_t)i);
        memset(nset, 0, sizeof(nset));
        for (int a = 0; a < 256; a++)
            for (int b = 0; b < 256; b++) {
                const float m = n[a] * 0.5f + n[b] * 0.5f;
                const int s = a + b;
                int k;
                for (k = 0; k < nset[s]; k++) if (set[s][k] == m) break;
                if (k == nset[s]) {
                    if (nset[s] >= MAXSET) { fprintf(stderr, "mean set overflow\n"); return 2; }
                    set[s][nset[s]++] = m;
                }
            }
        int maxs = 0; long long tot = 0;
        for (int s = 0; s < NS; s++) { if (nset[s] > maxs) maxs = nset[s]; tot += nset[s]; }
        printf("chroma the pair mean a/255 * .5 + b/255 * .5 takes at most %d values per byte sum (%.2f on average)\n", maxs, (double)tot / NS);
    }
    for (int plane = 1; plane <= 2; plane++) {
        const yuvfast::K F = yuvfast::constants422(plane);
        printf("plane %d k = %.9g %.9g %.9g  k0 = %.9g\n", plane, F.kr, F.kg, F.kb, F.k0);
        long long sums = 0, sums_flagged = 0, total = 0, flagged = 0, mism_flagged = 0, mism_unflagged = 0;
        double maxdev = 0.0;
        const int step = quick ? 8 : 1;
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : sums, sums_flagged, total, flagged, mism_flagged, mism_unflagged) reduction(max : maxdev)
        for (int sr = 0; sr < NS; sr += step)
            for (int sg = 0; sg < NS; sg++)
                for (int sb = 0; sb < NS; sb++) {
                    const float x = fast_x(plane, (float)sr, (float)sg, (float)sb);
                    bool flag;
                    const uint32_t got = fast_convert(plane, (float)sr, (float)sg, (float)sb, &flag);
                    const double xf = (double)x - GUARD;
                    sums++;
                    sums_flagged += flag;
                    for (int i = 0; i < nset[sr]; i++)
                        for (int j = 0; j < nset[sg]; j++)
                            for (int k = 0; k < nset[sb]; k++) {
                                float pre;
                                const uint32_t want = yuv_byte(set[sr][i], set[sg][j], set[sb][k], plane, &pre);
                                const double dev = fabs(xf - (double)pre);
                                if (dev > maxdev) maxdev = dev;
                                total++;
                                flagged += flag;
                                if (got != want) {
                                    if (flag) mism_flagged++; else mism_unflagged++;
                                }
                            }
                }
        printf("plane %d %lld sum triples, %lld combinations: flagged %.4f %% (of the sum triples %.4f %%), of them with another byte than the sequence's %lld, mismatches NOT flagged %lld; |fast - sequence| <= %.3g, guard band %.3g (%.2f x)\n",
               plane, sums, total, 100.0 * (double)flagged / (double)total, 100.0 * (double)sums_flagged / (double)sums, mism_flagged, mism_unflagged, maxdev, GUARD, GUARD / maxdev);
        if (mism_unflagged) bad = 1;
    }
    printf(bad ? "FAILED\n" : "OK: the pair fast path never disagrees with the reference sequence outside its guard band\n");
    return bad;
}
