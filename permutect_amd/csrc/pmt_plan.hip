// The group planners: which consecutive read sets share a workgroup of the read-set kernels.  On the host pmt_plan_groups, its
// variant for read sets beyond one workgroup (pmt_plan_groups_split), the order in which a batch packs fuller (pmt_pack_order) and
// everything the chunk loader needs of them in one call (pmt_prepare_chunk); on the device pmt_plan_groups_device.  The packing rule
// itself is pmt_plan.hpp's.
#include <hip/hip_runtime.h>
#include <string.h>

#include <thread>
#include <vector>

#include "pmt_jobs.hpp"
#include "pmt_plan.hpp"

// The next-fit walk over consecutive read sets: closed(b, ref, alt, tiles) for every group as it closes -- b the first set of the next
// group (num_variants after the last one), ref / alt the reads of the closed one, tiles the tile base behind it; false stops the walk.
template <typename Closed>
static bool walk_groups(const int32_t* ref_counts, const int32_t* alt_counts, int num_variants, Closed&& closed) {
    NextFit<long long> open;
    auto close = [&](int b) {
        const long long ref = open.ref, alt = open.alt;
        return closed(b, ref, alt, open.close());
    };
    for (int b = 0; b < num_variants; ++b) {
        const long long r = ref_counts[b], a = alt_counts[b];
        if (open.closes(r, a) && !close(b)) return false;
        open.add(r, a);
    }
    return open.sets == 0 || close(num_variants);
}

extern "C" int pmt_plan_groups(const int32_t* ref_counts, const int32_t* alt_counts, int32_t num_variants,
                               int32_t* group_start, int32_t* group_tile_base, int32_t* bad_variant) {
    if (!ref_counts || !alt_counts || !group_start || !group_tile_base || num_variants < 0) return PMT_E_INVALID;
    int groups = 0;
    group_start[0] = 0;
    group_tile_base[0] = 0;
    for (int b = 0; b < num_variants; ++b) {
        if (ref_counts[b] < 0 || alt_counts[b] < 0) return PMT_E_INVALID;
        if (!group_fits_reads<long long>(ref_counts[b], alt_counts[b])) {
            if (bad_variant) *bad_variant = b;
            return PMT_E_CAPACITY;
        }
    }
    walk_groups(ref_counts, alt_counts, num_variants, [&](int b, long long, long long, long long tiles) {
        ++groups;
        group_start[groups] = b;
        group_tile_base[groups] = (int32_t)tiles;
        return true;
    });
    return groups;
}

// ---- pmt_plan_groups ON THE DEVICE ---------------------------------------------------------------------------------------
// A DownsampledBatch keeps about half of its parent's reads (reference training/downsampler.py: a mixture of Beta fractions with mean
// one half), and how many is decided on the device (pmt_downsample_counts).  Until round 5 it ran on its PARENT's plan -- the parent's
// counts bound its own -- so every training step of the real loop launched the parent's ~3 400 workgroups with half-empty tiles and
// took the parent's time (a workgroup costs the same full or not).  Planning from the downsampled counts needs them where the
// planner runs; bringing them to the host would be a synchronisation per step, so the planner goes to the device instead:
// the batch is cut into chunks of consecutive variants, one thread packs a chunk exactly like pmt_plan_groups (the NextFit of
// pmt_plan.hpp; a chunk boundary closes a group: ~1 / 13 of a group per 256 variants lost), a prefix over the chunks' group and tile
// counts places their groups, and a second pass writes them.  The kernels take the group count from the device
// (PmtBatch.num_groups_dev) under a grid sized for a capacity.
// Next-fit over the same order never makes MORE groups when the items shrink (by induction the k-th boundary does not move left),
// so capacity = the parent's groups + the number of chunks; an overflow (a caller's wrong capacity) raises the fault word.
// One WAVE per chunk of 256 consecutive variants: its lanes load the chunk's counts coalesced (four registers per side), and the
// packing itself -- sequential by nature -- runs on the scalar unit, every lane in step, reading one variant's counts at a time out
// of the registers with v_readlane (~15 scalar instructions per variant: ~2 us per chunk).  Two launches: the chunks' group and
// tile counts, then (after a prefix over them, which every wave takes for itself) the groups written out.  The first version gave a
// chunk to one THREAD of a single workgroup, whose 256 dependent, uncoalesced loads took 174 us per 65 536-variant batch.
#define PLAN_CHUNK 256
#define PLAN_WAVES 4
// next-fit over the chunk [v0, v1), NextFit's statements (pmt_plan.hpp) written out: through the struct the two kernels took 15 % longer
// (profiles/host_split_device_asm_sha256.txt; tests/test_balancer_gpu.py holds this walk to the host's).  WRITE: groups g0 + 1 .. go to group_start / group_tile_base (lane 0 stores).  Wave-uniform throughout.
template <bool WRITE>
__device__ void plan_chunk_wave(const int* __restrict__ ro, const int* __restrict__ ao, int v0, int v1, int g0, int t0, int* __restrict__ group_start,
                                int* __restrict__ group_tile_base, int capacity, int& groups, int& tiles, int& bad) {
    const int lane = threadIdx.x & 63;
    int rc[PLAN_CHUNK / 64], ac[PLAN_CHUNK / 64];
#pragma unroll
    for (int k = 0; k < PLAN_CHUNK / 64; ++k) {
        const int b = v0 + 64 * k + lane;
        rc[k] = b < v1 ? ro[b + 1] - ro[b] : 0;
        ac[k] = b < v1 ? ao[b + 1] - ao[b] : 0;
    }
    int ref = 0, alt = 0, sets = 0, g = g0, t = t0;
    const int n = v1 - v0;
#pragma unroll
    for (int k = 0; k < PLAN_CHUNK / 64; ++k) {
        const int m = min(64, n - 64 * k);
        for (int l = 0; l < m; ++l) {
            const int r = __builtin_amdgcn_readlane(rc[k], l), a = __builtin_amdgcn_readlane(ac[k], l);
            if (!group_fits_reads(r, a)) bad = 1;  // (a read set beyond one workgroup: the caller's batch is not one for this planner)
            if (sets > 0 && (!group_fits_reads(ref + r, alt + a) || sets + 1 > PMT_GROUP_MAX_SETS)) {
                t += ((ref + 15) >> 4) + ((alt + 15) >> 4);
                ++g;
                if (WRITE && g <= capacity && lane == 0) { group_start[g] = v0 + 64 * k + l; group_tile_base[g] = t; }
                ref = alt = 0;
                sets = 0;
            }
            ref += r; alt += a; ++sets;
        }
    }
    if (sets > 0) {
        t += ((ref + 15) >> 4) + ((alt + 15) >> 4);
        ++g;
        if (WRITE && g <= capacity && lane == 0) { group_start[g] = v1; group_tile_base[g] = t; }
    }
    groups = g - g0; tiles = t - t0;
}
// launch 1: per chunk (groups, tiles) -> counts[2 c], counts[2 c + 1]
__global__ __launch_bounds__(64 * PLAN_WAVES) void pmt_plan_count_kernel(const int* __restrict__ ro, const int* __restrict__ ao, int n, int nchunks,
                                                                          int* __restrict__ counts) {
    const int c = blockIdx.x * PLAN_WAVES + (threadIdx.x >> 6);
    if (c >= nchunks) return;
    int groups = 0, tiles = 0, bad = 0;
    plan_chunk_wave<false>(ro, ao, c * PLAN_CHUNK, min(n, (c + 1) * PLAN_CHUNK), 0, 0, nullptr, nullptr, 0, groups, tiles, bad);
    if ((threadIdx.x & 63) == 0) {
        counts[2 * c] = groups;
        counts[2 * c + 1] = tiles | (bad ? (1 << 30) : 0);
    }
}
// launch 2: every wave sums the chunks in front of its own (coalesced, a wave reduction), then packs its chunk again, writing
__global__ __launch_bounds__(64 * PLAN_WAVES) void pmt_plan_write_kernel(const int* __restrict__ ro, const int* __restrict__ ao, int n, int nchunks,
                                                                          const int* __restrict__ counts, int* __restrict__ group_start,
                                                                          int* __restrict__ group_tile_base, int capacity,
                                                                          int* __restrict__ num_groups_dev, int* __restrict__ fault) {
    const int c = blockIdx.x * PLAN_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= nchunks) return;
    int g0 = 0, t0 = 0, total = 0, bad = 0;
    for (int i = lane; i < nchunks; i += 64) {
        const int gi = counts[2 * i], ti = counts[2 * i + 1];
        bad |= ti >> 30;
        total += gi;
        if (i < c) { g0 += gi; t0 += ti & ((1 << 30) - 1); }
    }
    for (int d = 32; d > 0; d >>= 1) {
        g0 += __shfl_xor(g0, d); t0 += __shfl_xor(t0, d); total += __shfl_xor(total, d); bad |= __shfl_xor(bad, d);
    }
    if (c == 0 && lane == 0) {
        group_start[0] = 0;
        group_tile_base[0] = 0;
        num_groups_dev[0] = min(total, capacity);
        if ((total > capacity || bad) && fault != nullptr) atomicOr(fault, PMT_FAULT_PLAN);
    }
    int groups = 0, tiles = 0, bad2 = 0;
    plan_chunk_wave<true>(ro, ao, c * PLAN_CHUNK, min(n, (c + 1) * PLAN_CHUNK), g0, t0, group_start, group_tile_base, capacity, groups, tiles, bad2);
}

extern "C" int pmt_plan_device_chunks(int32_t num_variants) {  // how many chunks pmt_plan_groups_device cuts a batch into (capacity = the parent's groups + this)
    return (num_variants + PLAN_CHUNK - 1) / PLAN_CHUNK;
}
extern "C" int pmt_plan_groups_device(const int32_t* ref_offsets, const int32_t* alt_offsets, int32_t num_variants, int32_t* group_start,
                                      int32_t* group_tile_base, int32_t capacity, int32_t* num_groups_dev, int32_t* fault, int32_t* scratch,
                                      void* stream) {
    if (!ref_offsets || !alt_offsets || !group_start || !group_tile_base || !num_groups_dev || !scratch || num_variants < 1 || capacity < 1) return PMT_E_INVALID;
    const int nchunks = pmt_plan_device_chunks(num_variants);
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((nchunks + PLAN_WAVES - 1) / PLAN_WAVES), block(64 * PLAN_WAVES);
    hipLaunchKernelGGL(pmt_plan_count_kernel, grid, block, 0, s, ref_offsets, alt_offsets, num_variants, nchunks, scratch);
    hipLaunchKernelGGL(pmt_plan_write_kernel, grid, block, 0, s, ref_offsets, alt_offsets, num_variants, nchunks, scratch, group_start, group_tile_base,
                       capacity, num_groups_dev, fault);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}

// An ORDER of the batch's variants in which pmt_plan_groups packs fuller groups.  A workgroup costs the same whether its
// 16 tile slots are full or not, and the kernels run in rounds of (CUs x workgroups per CU) workgroups, so the number of
// groups is what the batch costs.  Taking the variants as they come fills a group to ~91 % (the next variant often does not
// fit the last wave of one side); here the group under construction may take, out of the next `window` unplaced variants,
// the first one that still fits: ~97 % (65 536 WGS-shaped variants: 3 643 -> 3 414 groups).  The caller composes the
// batch in the returned order (order[i] = index of the variant to put at position i); oversized variants are emitted when they
// become the oldest unplaced one and are left to pmt_plan_groups_split.
extern "C" int pmt_pack_order(const int32_t* ref_counts, const int32_t* alt_counts, int32_t num_variants, int32_t window,
                              int32_t* order) {
    if (!ref_counts || !alt_counts || !order || num_variants < 0 || window < 1) return PMT_E_INVALID;
    for (int i = 0; i < num_variants; ++i)
        if (ref_counts[i] < 0 || alt_counts[i] < 0) return PMT_E_INVALID;
    // `cand`: the (at most `window`) oldest unplaced variants, oldest first; `next`: the first variant not yet in it
    std::vector<int> cand;
    cand.reserve((size_t)window);
    int next = 0, placed = 0;
    auto refill = [&] {
        while ((int)cand.size() < window && next < num_variants) cand.push_back(next++);
    };
    refill();
    while (!cand.empty()) {
        NextFit<long long> open;
        for (;;) {
            size_t found = cand.size();
            for (size_t c = 0; c < cand.size(); ++c) {
                const int i = cand[c];
                const long long r = ref_counts[i], a = alt_counts[i];
                // an oversized variant is a group (or several) of its own: it goes when it is the oldest one and the group is empty
                const bool oversized = !group_fits_reads(r, a);
                if (oversized ? (open.sets == 0 && c == 0) : open.takes(r, a)) {
                    found = c;
                    break;
                }
            }
            if (found == cand.size()) break;
            const int v = cand[found];
            cand.erase(cand.begin() + (long)found);
            order[placed++] = v;
            open.add(ref_counts[v], alt_counts[v]);
            refill();
            if (!group_fits_reads<long long>(ref_counts[v], alt_counts[v])) break;  // (the oversized one closes its group)
        }
        if (open.sets == 0 && !cand.empty()) {  // the oldest is oversized but an ordinary group was being asked for: cannot happen
            order[placed++] = cand[0];          // with sets == 0 (it would have been taken); kept as a guard against a stall
            cand.erase(cand.begin());
            refill();
        }
    }
    return placed == num_variants ? PMT_OK : PMT_E_INVALID;
}

// The same for consecutive batches of `batch` variants at once (a chunk of the dataset), on `threads` host threads and
// outside the Python GIL: order[k * batch + i] = position, within the whole array, of the variant to put at place i of batch k.
extern "C" int pmt_pack_order_batches(const int32_t* ref_counts, const int32_t* alt_counts, int32_t num_variants, int32_t batch,
                                      int32_t window, int32_t threads, int32_t* order) {
    if (!ref_counts || !alt_counts || !order || num_variants < 0 || batch < 1 || window < 1) return PMT_E_INVALID;
    const int nb = (num_variants + batch - 1) / batch;
    std::vector<int> rc((size_t)(nb > 0 ? nb : 1), PMT_OK);
    for_each_job(threads, nb, [&](int k) {
        const int lo = k * batch, n = (lo + batch <= num_variants ? batch : num_variants - lo);
        rc[k] = pmt_pack_order(ref_counts + lo, alt_counts + lo, n, window, order + lo);
        for (int i = 0; i < n; ++i) order[lo + i] += lo;
    });
    for (int k = 0; k < nb; ++k)
        if (rc[k] != PMT_OK) return rc[k];
    return PMT_OK;
}

// Everything the device chunk loader needs from the HOST for one chunk of the dataset, in one call outside the Python GIL
// (reference data/reads_dataset.py:141-196 does the same bookkeeping one Datum at a time in Python): the chunk's read counts,
// the order in which its variants are consumed (shuffled or not, then ordered inside every batch for the group packer), and
// every batch's group plan.  Returns the number of batches, PMT_E_CAPACITY when some read set needs the split plan (the caller
// then plans that chunk batch by batch with pmt_plan_groups_split), or another error.
//   ints / row_stride / ref_col / alt_col: the dataset's int16 table (row stride in elements) and its two count columns
//   ref_host, alt_host [n]: out, counts in chunk order
//   ids [n]: out, variant ids (0 .. n-1) in consumption order: batch k is ids[k * batch, (k + 1) * batch)
//   plans: out, per batch [group_start (g + 1 ints) | group_tile_base (g + 1 ints)], packed back to back; capacity in ints
//   batch_info [nb][4]: out, {offset of the batch's plan in `plans`, groups g, total tiles, total reads}
static inline uint64_t splitmix64(uint64_t& x) {
    uint64_t z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
extern "C" int pmt_prepare_chunk(const int16_t* ints, int64_t row_stride, int32_t ref_col, int32_t alt_col, int32_t n, int32_t shuffle,
                                 uint64_t seed, int32_t batch, int32_t window, int32_t threads, int32_t* ref_host, int32_t* alt_host,
                                 int64_t* ids, int32_t* plans, int64_t plans_capacity, int32_t* batch_info, int32_t* offsets) {
    if (!ints || !ref_host || !alt_host || !ids || !plans || !batch_info || n < 0 || batch < 1 || window < 1 || row_stride < 1) return PMT_E_INVALID;
    const int nb = (n + batch - 1) / batch;
    if (threads < 1) threads = 1;
    // the counts: two int16 per 100-byte row (a cache line per variant), gathered by all threads; the shuffle meanwhile
    std::thread shuffler([&] {
        for (int i = 0; i < n; ++i) ids[i] = i;
        if (shuffle) {  // Fisher-Yates on a splitmix64 stream; j = floor(u * (i + 1) / 2^64): unbiased to 2^-45 for i < 2^19
            uint64_t state = seed;
            for (int i = n - 1; i > 0; --i) {
                const int j = (int)(((unsigned __int128)splitmix64(state) * (uint64_t)(i + 1)) >> 64);
                const int64_t t = ids[i]; ids[i] = ids[j]; ids[j] = t;
            }
        }
    });
    const int slices = threads * 4;
    for_each_job(threads, slices, [&](int sl) {
        const int lo = (int)((long long)n * sl / slices), hi = (int)((long long)n * (sl + 1) / slices);
        for (int i = lo; i < hi; ++i) {
            ref_host[i] = ints[(size_t)i * row_stride + ref_col];
            alt_host[i] = ints[(size_t)i * row_stride + alt_col];
        }
    });
    shuffler.join();
    for (int i = 0; i < n; ++i)
        if (ref_host[i] < 0 || alt_host[i] < 0) return PMT_E_INVALID;
    // Packing order inside every batch (pmt_pack_order is sequential: ~60 ns per variant).  A large batch is ordered in two
    // halves on two threads -- the only cost is one more partly filled group where the halves meet.
    const int parts = batch >= 16384 ? 2 : 1;
    std::vector<int> rc((size_t)(nb > 0 ? nb : 1) * parts, PMT_OK);
    for_each_job(threads, nb * parts, [&](int job) {
        const int k = job / parts, part = job % parts;
        const int blo = k * batch, m = (blo + batch <= n ? batch : n - blo);
        const int lo = blo + (int)((long long)m * part / parts), cnt = blo + (int)((long long)m * (part + 1) / parts) - lo;
        std::vector<int32_t> r((size_t)cnt), a((size_t)cnt), order((size_t)cnt);
        std::vector<int64_t> tmp((size_t)cnt);
        for (int i = 0; i < cnt; ++i) { r[i] = ref_host[ids[lo + i]]; a[i] = alt_host[ids[lo + i]]; }
        const int e = pmt_pack_order(r.data(), a.data(), cnt, window, order.data());
        if (e != PMT_OK) { rc[job] = e; return; }
        for (int i = 0; i < cnt; ++i) tmp[i] = ids[lo + order[i]];
        for (int i = 0; i < cnt; ++i) ids[lo + i] = tmp[i];
    });
    for (size_t j = 0; j < rc.size(); ++j)
        if (rc[j] != PMT_OK) return rc[j];
    // every batch plans into its own slot of a scratch area (its size is not known beforehand), packed together afterwards
    const size_t slot = 2 * ((size_t)batch + 1);
    std::vector<int32_t> scratch((size_t)(nb > 0 ? nb : 1) * slot);
    std::vector<int> groups((size_t)(nb > 0 ? nb : 1), 0);
    for_each_job(threads, nb, [&](int k) {
        const int lo = k * batch, m = (lo + batch <= n ? batch : n - lo);
        std::vector<int32_t> r((size_t)m), a((size_t)m);
        long long reads = 0;
        for (int i = 0; i < m; ++i) { r[i] = ref_host[ids[lo + i]]; a[i] = alt_host[ids[lo + i]]; reads += (long long)r[i] + a[i]; }
        int32_t* gs = scratch.data() + (size_t)k * slot;
        int32_t bad = -1;
        groups[k] = pmt_plan_groups(r.data(), a.data(), m, gs, gs + batch + 1, &bad);  // >= 0: the number of groups
        batch_info[4 * k + 3] = (int32_t)reads;
        if (offsets != nullptr) {  // the exclusive scans of the batch's counts, in its consumption order (pmt_compose_batch_planned)
            int32_t* ro = offsets + (size_t)k * 2 * ((size_t)batch + 1);
            int32_t* ao = ro + batch + 1;
            int32_t rs = 0, as = 0;
            for (int i = 0; i < m; ++i) { ro[i] = rs; ao[i] = as; rs += r[i]; as += a[i]; }
            ro[m] = rs; ao[m] = as;
        }
    });
    int64_t at = 0;
    for (int k = 0; k < nb; ++k) {
        if (groups[k] < 0) return groups[k];
        const int g = groups[k];
        if (at + 2 * ((int64_t)g + 1) > plans_capacity) return PMT_E_WORKSPACE;
        const int32_t* gs = scratch.data() + (size_t)k * slot;
        const int32_t* gt = gs + batch + 1;
        memcpy(plans + at, gs, sizeof(int32_t) * ((size_t)g + 1));
        memcpy(plans + at + g + 1, gt, sizeof(int32_t) * ((size_t)g + 1));
        batch_info[4 * k] = (int32_t)at; batch_info[4 * k + 1] = g; batch_info[4 * k + 2] = gt[g];
        at += 2 * ((int64_t)g + 1);
    }
    return nb;
}

extern "C" int pmt_plan_groups_split(const int32_t* ref_counts, const int32_t* alt_counts, int32_t num_variants, int32_t* span,
                                     int32_t* tile_base, int32_t max_groups, int32_t* needs_layered) {
    if (!ref_counts || !alt_counts || !span || !tile_base || !needs_layered || num_variants < 0 || max_groups < 1) return PMT_E_INVALID;
    const long long per = PMT_GROUP_TILES / PMT_GROUP_WAVES;
    int g = 0;
    long long tiles = 0;
    *needs_layered = 0;
    auto emit = [&](long long v0, long long v1, long long rb, long long re, long long ab, long long ae) {
        if (g >= max_groups) return false;
        int32_t* sp = span + 6 * (size_t)g;
        sp[0] = (int32_t)v0; sp[1] = (int32_t)v1; sp[2] = (int32_t)rb; sp[3] = (int32_t)re; sp[4] = (int32_t)ab; sp[5] = (int32_t)ae;
        tile_base[g] = (int32_t)tiles;
        tiles += (re - rb + 15) / 16 + (ae - ab + 15) / 16;
        ++g;
        return true;
    };
    bool oversized = false;
    for (int b = 0; b < num_variants; ++b) {
        if (ref_counts[b] < 0 || alt_counts[b] < 0) return PMT_E_INVALID;
        oversized = oversized || !group_fits_reads<long long>(ref_counts[b], alt_counts[b]);
    }
    long long ref_row = 0, alt_row = 0;         // exclusive scans so far
    if (!oversized) {  // every set fits a workgroup: whole sets per group, the walk of pmt_plan_groups
        int v0 = 0;
        const bool room = walk_groups(ref_counts, alt_counts, num_variants, [&](int b, long long ref, long long alt, long long) {
            if (!emit(v0, b, ref_row, ref_row + ref, alt_row, alt_row + alt)) return false;
            v0 = b; ref_row += ref; alt_row += alt;
            return true;
        });
        if (!room) return PMT_E_WORKSPACE;
        tile_base[g] = (int32_t)tiles;
        return g;
    }
    // Some set exceeds a workgroup: the batch runs layered, where a group may hold ANY contiguous run of ref rows and of alt
    // rows (per-set sums are joined in HBM).  So the rows are STREAMED into groups -- a set's ref rows, then its alt rows, the
    // next set right behind -- and a group is closed only when nothing more fits: ~ceil(tiles / 16) groups instead of one
    // partly empty last group per oversized set (600-read sets: 3 groups of 16 tile slots for 38 tiles each before).
    *needs_layered = 1;
    auto waves_of = [&](long long rows) { return ((rows + 15) / 16 + per - 1) / per; };
    long long g_v0 = 0, g_rb = 0, g_ab = 0, gref = 0, galt = 0;
    int sets = 0;
    bool open = false;
    for (int b = 0; b < num_variants; ++b) {
        const long long r = ref_counts[b], a = alt_counts[b];
        long long rdone = 0, adone = 0;
        bool counted = false;  // set b has rows in the open group
        while (rdone < r || adone < a) {
            if (!open) {
                g_v0 = b; g_rb = ref_row + rdone; g_ab = alt_row + adone; gref = galt = 0; sets = 0;
                open = true; counted = false;
            }
            bool placed = false;
            if (counted || sets < PMT_GROUP_MAX_SETS) {
                if (rdone < r) {
                    const long long room = (PMT_GROUP_WAVES - waves_of(galt)) * per * 16 - gref;
                    const long long x = (r - rdone) < room ? (r - rdone) : room;
                    if (x > 0) { gref += x; rdone += x; placed = true; }
                }
                if (rdone == r && adone < a) {
                    const long long room = (PMT_GROUP_WAVES - waves_of(gref)) * per * 16 - galt;
                    const long long y = (a - adone) < room ? (a - adone) : room;
                    if (y > 0) { galt += y; adone += y; placed = true; }
                }
            }
            if (placed && !counted) { counted = true; ++sets; }
            if (rdone < r || adone < a) {  // the group is full (or has its sets): close it; set b continues in the next one
                if (!emit(g_v0, counted ? b + 1 : b, g_rb, g_rb + gref, g_ab, g_ab + galt)) return PMT_E_WORKSPACE;
                open = false;
            }
        }
        ref_row += r; alt_row += a;
    }
    if (open && gref + galt > 0 && !emit(g_v0, num_variants, g_rb, g_rb + gref, g_ab, g_ab + galt)) return PMT_E_WORKSPACE;
    tile_base[g] = (int32_t)tiles;
    return g;
}
