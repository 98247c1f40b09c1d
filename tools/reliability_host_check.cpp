// Host-side check of acg_reliability (include/acgan_verif.h) for a sanitizer build: every refusal in its documented order and
// the workspace arithmetic, nothing that launches.  No GPU is needed or touched: a refused call returns before any HIP call.
// Build and run on a CPU box, from the repository root:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       domain-transfer-gan_amd/csrc/fss.hip domain-transfer-gan_amd/csrc/elementwise.hip tools/reliability_host_check.cpp \
//       -o /tmp/reliability_host_check && /tmp/reliability_host_check
//
// Prints "reliability_host_check ok" and exits 0; a wrong status or message exits 1, and the sanitizers report on their own.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/acgan_hip.h"
#include "../include/acgan_verif.h"

static int failures = 0;

static void expect(int rc, int want, const char *word, const char *what)
{
    const char *msg = acg_last_error();
    if (rc != want || strncmp(msg, "acg_reliability", 15) != 0 || strstr(msg, word) == nullptr) {
        printf("FAIL %s: status %d (want %d), message \"%s\" (want \"%s\")\n", what, rc, want, msg, word);
        ++failures;
    }
}

static size_t up16(size_t n) { return (n + 15) / 16 * 16; }
static size_t planes(size_t n, int H, int W)
{
    const size_t WW = (size_t)(W + 63) / 64;
    return up16(n * H * WW * 8) + up16(n * H * (WW + 1) * 2);
}

int main()
{
    if (acg_verif_version() != ACG_VERIF_VERSION) {
        printf("FAIL version %d\n", acg_verif_version());
        return 1;
    }
    // the buffers are host memory of a few bytes: a refusal that read or wrote through them would be the sanitizer's finding
    float *x = (float *)malloc(4), *thr = (float *)malloc(4);
    long long *table = (long long *)malloc(8);
    void *ws = aligned_alloc(16, 16);
    int win[9] = {1, 3, 5, 7, 9, 11, 13, 15, 17};
    const long long R = 4096;
    struct Args {
        const float *x, *y;
        int rows, per, C, H, W;
        long long xr;
        int xp;
        long long xc, yr;
        int yp;
        long long yc;
        const float *thr;
        int T;
        const int *win;
        int nw;
        long long *table;
        void *ws;
        size_t bytes;
    } a = {nullptr, nullptr, 0, 0, 0, 0, 1025, 0, 1, R, R, 1, -1, nullptr, 9, nullptr, 9, nullptr, (char *)ws + 8, 0};
    auto call = [&]() {
        return acg_reliability(a.x, a.y, a.rows, a.per, a.C, a.H, a.W, a.xr, a.xp, a.xc, a.yr, a.yp, a.yc, a.thr, a.T, a.win, a.nw, a.table,
                               a.ws, a.bytes, nullptr);
    };
    // everything is wrong at once; each refusal is mended in the documented order and shows the next
    expect(call(), -1, "rows >= 1", "rows"), a.rows = 2;
    expect(call(), -1, "C >= 1", "C"), a.C = 1;
    expect(call(), -1, "strides", "x stride"), a.xr = R;
    expect(call(), -1, "strides", "y stride"), a.yc = R;
    expect(call(), -1, "x_per_y", "x_per_y 0"), a.per = 3;
    expect(call(), -1, "x_per_y", "x_per_y 3 of 2"), a.per = 65, a.rows = 130;
    expect(call(), -1, "x_per_y", "x_per_y 65"), a.per = 1, a.rows = 2, a.x = x;
    expect(call(), -1, "null", "y"), a.y = x;
    expect(call(), -1, "null", "thr"), a.thr = thr;
    expect(call(), -1, "null", "windows"), a.win = win;
    expect(call(), -1, "null", "table"), a.table = table;
    expect(call(), -1, "H x W", "H"), a.H = 64;
    expect(call(), -1, "H x W", "W"), a.W = 64;
    expect(call(), -1, "thresholds", "T 9"), a.T = 0;
    expect(call(), -1, "thresholds", "T 0"), a.T = 1;
    expect(call(), -1, "windows (nw=", "nw 9"), a.nw = 0;
    expect(call(), -1, "windows (nw=", "nw 0"), a.nw = 2, win[1] = 4;
    expect(call(), -1, "odd", "even window"), win[1] = 67;
    expect(call(), -1, "odd", "window 67"), win[1] = -3;
    expect(call(), -1, "odd", "window -3"), win[0] = 0, win[1] = 3;
    expect(call(), -1, "odd", "window 0"), win[0] = 1, win[1] = 65;
    const size_t need = acg_reliability_workspace_bytes(2, 1, 1, 64, 64, 1, 2);
    expect(call(), -2, "workspace too small", "no bytes"), a.bytes = need - 1;
    expect(call(), -2, "workspace too small", "short"), a.bytes = need;
    expect(call(), -1, "aligned", "misaligned");
    a.ws = nullptr;
    expect(call(), -2, "workspace too small", "missing");
    // the query: the planes of x and of y, whatever the windows; 0 for what the call refuses
    if (need != 2 * planes(2, 64, 64)) printf("FAIL need %zu\n", need), ++failures;
    const int sizes[][2] = {{1, 1}, {5, 7}, {64, 64}, {65, 130}, {321, 321}, {1024, 1024}, {1, 1024}, {1024, 1}};
    for (const auto &s : sizes) {
        const int H = s[0], W = s[1];
        if (acg_reliability_workspace_bytes(4, 2, 3, H, W, 3, 6) != planes(36, H, W) + planes(18, H, W)) printf("FAIL %d x %d\n", H, W), ++failures;
        if (acg_reliability_workspace_bytes(64, 64, 1, H, W, 8, 8) != planes(512, H, W) + planes(8, H, W)) printf("FAIL %d x %d M\n", H, W), ++failures;
    }
    // the largest accepted plane counts: no overflow in the byte arithmetic
    if (acg_reliability_workspace_bytes(262143, 1, 1, 1024, 1024, 8, 8) == 0) printf("FAIL large\n"), ++failures;
    const int bad[][7] = {{0, 1, 1, 8, 8, 1, 1}, {2, 1, 0, 8, 8, 1, 1}, {2, 0, 1, 8, 8, 1, 1}, {130, 65, 1, 8, 8, 1, 1}, {6, 4, 1, 8, 8, 1, 1},
                          {2, 1, 1, 0, 8, 1, 1}, {2, 1, 1, 8, 0, 1, 1}, {2, 1, 1, 1025, 8, 1, 1}, {2, 1, 1, 8, 1025, 1, 1}, {2, 1, 1, 8, 8, 0, 1},
                          {2, 1, 1, 8, 8, 9, 1}, {2, 1, 1, 8, 8, 1, 0}, {2, 1, 1, 8, 8, 1, 9}, {1 << 30, 1, 4, 8, 8, 1, 1}, {-1, 1, 1, 8, 8, 1, 1},
                          {0x7fffffff, 1, 1, 1024, 8, 1, 1}, {2, -1, 1, 8, 8, 1, 1}, {2, 1, -1, 8, 8, 1, 1}, {2, 1, 1, -8, 8, 1, 1}};
    for (const auto &b : bad)
        if (acg_reliability_workspace_bytes(b[0], b[1], b[2], b[3], b[4], b[5], b[6]) != 0) printf("FAIL query of a refused size (rows %d)\n", b[0]), ++failures;
    free(x), free(thr), free(table), free(ws);
    if (failures) return 1;
    printf("reliability_host_check ok\n");
    return 0;
}
