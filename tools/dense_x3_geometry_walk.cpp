// dense_x3_geometry_walk.cpp — a stand-alone host program over the geometry and validation helpers of
// csrc/dense_tiled_x3.hip, meant to be built with the host sanitizers (no GPU is touched: no launch is made):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -x hip \
//         deeptables_amd/csrc/dense_tiled_x3.hip tools/dense_x3_geometry_walk.cpp -o dense_x3_geometry_walk
// It walks dt_dense_x3_supported / _workspace_bytes / _geometry over a grid of shapes (N K > 2^31 included) and checks that
// every product's tiles and splits cover its output and its contraction exactly once; exit status 0 = all held.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "../include/dt_hip.h"

namespace dt {
static char g_err[512];
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
}  // namespace dt

static int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

int main() {
    const int Ns[] = {-1, 0, 1, 31, 32, 33, 255, 256, 257, 4100, 8192, 65536, 212992, 300000, 2147483647};
    const int Ks[] = {-3, 0, 1, 31, 32, 33, 64, 1204, 2912, 10413, 65535 * 64, 65535 * 64 + 1, 2147483647};
    const int Ms[] = {-2, 0, 1, 2, 3, 63, 64, 65, 128, 832, 1300, 65535 * 64, 65535 * 64 + 1};
    const int modes[] = {0, DT_DENSE_X3, DT_DENSE_BF16, 3, -1};
    long checked = 0, refused = 0;
    for (int N : Ns) for (int K : Ks) for (int M : Ms) for (int mode : modes) {
        const int ok = dt_dense_x3_supported(N, K, M, mode);
        const bool want = (mode == DT_DENSE_X3 || mode == DT_DENSE_BF16) && N > 0 && K > 0 && M >= 2 &&
                          cdiv(K, 64) <= 65535 && cdiv(M, 64) <= 65535;
        if ((ok != 0) != want) { printf("supported(%d,%d,%d,%d) = %d\n", N, K, M, mode, ok); return 1; }
        if (dt_dense_x3_workspace_bytes(N, K, M, mode) < 0) { printf("workspace(%d,%d,%d,%d) < 0\n", N, K, M, mode); return 1; }
        for (int product = -1; product <= 3; ++product) {
            int tr = -7, tc = -7, sp = -7, per = -7;
            const int rc = dt_dense_x3_geometry(N, K, M, mode, product, &tr, &tc, &sp, &per);
            if (!want || product < 0 || product > 2) {
                if (rc == DT_OK || tr != -7 || tc != -7 || sp != -7 || per != -7) {
                    printf("geometry(%d,%d,%d,%d,%d) = %d outside the domain\n", N, K, M, mode, product, rc);
                    return 1;
                }
                ++refused;
                continue;
            }
            const int64_t Kc = product == 0 ? K : product == 1 ? M : N;
            const int64_t steps = cdiv(Kc, 32);
            const bool fine = rc == DT_OK && tr == tc && (tr == 64 || tr == 128) && sp >= 1 && per >= 1 &&
                              (int64_t)(sp - 1) * per < steps && steps <= (int64_t)sp * per && (sp == 1 || product == 2) &&
                              sp <= 65535 && dt_dense_x3_geometry(N, K, M, mode, product, nullptr, nullptr, nullptr, nullptr) == DT_OK;
            if (!fine) {
                printf("geometry(%d,%d,%d,%d,%d) = %d: tile %d x %d, %d splits of %d steps\n", N, K, M, mode, product, rc, tr, tc,
                       sp, per);
                return 1;
            }
            ++checked;
        }
    }
    printf("dense_x3 geometry walk: %ld launches' geometry checked, %ld requests refused\n", checked, refused);
    return 0;
}
