// body(j) for j in [0, jobs) on up to `threads` host threads (thread t takes jobs t, t + threads, ...), inline when one suffices: the
// one job runner of the host code that works outside the Python GIL (pmt_plan.hip: pmt_pack_order_batches, pmt_prepare_chunk;
// pmt_host.hip: pmt_host_copy, pmt_host_copy_rows).
#pragma once
#include <thread>
#include <vector>

template <typename Body>
static void for_each_job(int threads, int jobs, Body&& body) {
    const int nt = threads < jobs ? threads : jobs;
    if (nt <= 1) {
        for (int j = 0; j < jobs; ++j) body(j);
        return;
    }
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; ++t)
        pool.emplace_back([&body, t, nt, jobs] { for (int j = t; j < jobs; j += nt) body(j); });
    for (auto& th : pool) th.join();
}
