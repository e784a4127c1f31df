// The host planners and the staging copies under AddressSanitizer + UBSan, stand-alone (no kernel is launched, no GPU is needed):
// every array on the heap at its exact size, the small inputs of tests/test_plan_cpu.py.  From the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Iinclude scripts/plan_sanitize.cpp \
//         permutect_amd/csrc/pmt_plan.hip permutect_amd/csrc/pmt_host.hip -o /tmp/plan_sanitize && /tmp/plan_sanitize
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "permutect_amd.h"

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static int run_case(const std::vector<int32_t>& ref, const std::vector<int32_t>& alt, bool whole_sets) {
    const int n = (int)ref.size(), batch = 256, nb = (n + batch - 1) / batch;
    std::vector<int32_t> gs(n + 1), gt(n + 1), order(n), span(6 * (size_t)(2 * n + 16)), tb(2 * n + 17);
    int32_t bad = -1, layered = -1;
    const int g = pmt_plan_groups(ref.data(), alt.data(), n, gs.data(), gt.data(), &bad);
    CHECK(whole_sets ? g >= 0 : g == PMT_E_CAPACITY);
    const int g2 = pmt_plan_groups_split(ref.data(), alt.data(), n, span.data(), tb.data(), 2 * n + 16, &layered);
    CHECK(g2 >= 0 && (!whole_sets || (g2 == g && layered == 0)));
    if (g2 > 0) CHECK(pmt_plan_groups_split(ref.data(), alt.data(), n, span.data(), tb.data(), g2, &layered) == g2);  // exactly enough room
    CHECK(pmt_pack_order(ref.data(), alt.data(), n, 64, order.data()) == PMT_OK);
    CHECK(pmt_pack_order_batches(ref.data(), alt.data(), n, batch, 64, 3, order.data()) == PMT_OK);
    std::vector<int16_t> ints((size_t)n * 50, 0);
    for (int i = 0; i < n; ++i) { ints[(size_t)i * 50] = (int16_t)ref[i]; ints[(size_t)i * 50 + 1] = (int16_t)alt[i]; }
    std::vector<int32_t> rh(n), ah(n), plans(2 * (size_t)(n + nb)), info(4 * (size_t)nb), offsets((size_t)nb * 2 * (batch + 1));
    std::vector<int64_t> ids(n);
    for (int threads : {1, 8}) {
        const int rc = pmt_prepare_chunk(ints.data(), 50, 0, 1, n, 1, 9, batch, 64, threads, rh.data(), ah.data(), ids.data(), plans.data(),
                                         (int64_t)plans.size(), info.data(), offsets.data());
        CHECK(whole_sets ? rc == nb : rc == PMT_E_CAPACITY);
    }
    return 0;
}

int main() {
    std::srand(20);
    const int n = 2000;
    std::vector<int32_t> ref(n), alt(n);
    for (int i = 0; i < n; ++i) { ref[i] = std::rand() % 11; alt[i] = 1 + std::rand() % 15; }
    if (run_case(ref, alt, true)) return 1;                                                        // WGS-shaped
    if (run_case(std::vector<int32_t>(200, 0), std::vector<int32_t>(200, 1), true)) return 1;      // the 64-set limit alone
    if (run_case(std::vector<int32_t>(n, 128), std::vector<int32_t>(n, 128), true)) return 1;      // one set fills every wave
    ref[17] = 290; alt[400] = 310;
    if (run_case(ref, alt, false)) return 1;                                                       // oversized sets among small ones
    if (run_case({3}, {4}, true)) return 1;
    const size_t bytes = 5 * ((size_t)1 << 20) + 13;
    std::vector<char> src(bytes, 7), dst(bytes);
    const int64_t row_bytes = 100;
    for (int threads : {1, 8}) {
        CHECK(pmt_host_copy(dst.data(), src.data(), bytes, threads) == PMT_OK && std::memcmp(dst.data(), src.data(), bytes) == 0);
        for (int64_t rows : {9001, 30001}) {  // (30 001 rows: above 2 MiB, so more than one part)
            std::vector<char> rsrc((size_t)(rows * row_bytes), 5), rdst((size_t)(rows * row_bytes));
            CHECK(pmt_host_copy_rows(rdst.data(), rsrc.data(), rows, row_bytes, 0, 4, threads) == PMT_OK);
            CHECK(rdst[0] == 0 && rdst[3] == 0 && rdst[4] == 5 && rdst[(size_t)((rows - 1) * row_bytes)] == 0 && rdst.back() == 5);
        }
    }
    std::printf("plan_sanitize: clean\n");
    return 0;
}
