// stream_pool.hip -- where an engine's stream comes from: the per-device pool of streams created back to back (so that the
// stages of a pipeline sit on different front-end pipes), its self-check, and the HPS_CU_MASKS diagnostic.  Nothing of the
// reference is restated here.  Owns create_engine_stream / return_engine_stream (Engine::create, ~Engine) and
// hps_stream_pool_shared_pairs.
#include "common.h"
#include "engine.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

// the engines' stream pool (see create_engine_stream)
namespace {
std::mutex g_pool_mutex;
std::map<int, std::vector<hipStream_t>> g_stream_pool;      // device -> streams not in use
std::map<int, bool> g_pool_made;
}

namespace hps {

// HPS_CU_MASKS="lo-hi[+lo-hi...],..." (diagnostic): the j-th engine created in this process runs its stream on the compute
// units of entry j % n only (hipExtStreamCreateWithCUMask).  Bit i of a mask is compute unit i / 8 of XCD i % 8 on this GPU (the
// driver deals the bits round the XCDs first), so ranges that are multiples of 8 wide take the same number of CUs from every XCD.
//
// Default: the engines' streams come from a small per-device POOL whose streams are created back to back the first time an
// engine is created on the device.  Why: the runtime gives every stream a hardware queue when it is first used, hardware
// queues go to the 4 pipes of the compute front end in the order they are created (queue k of the PROCESS on pipe k mod 4),
// and two queues on one pipe do not overlap chains of short dependent kernels (the multigrid's ~30 launches of 5-10 us): two
// stages whose queues are 4 apart take turns.  Measured on MI355X (scripts/ubench/queue_pairs.hip; profiles/r05_queue_pairs.txt,
// r05_stage_queues.txt): three stages whose engines were created AFTER the ring's two streams sat on queues 1, 5, 6 and made
// 1700 slices/s, created before them (queues 1, 3, 4) 2186.  With the pool the stages' queues are consecutive whatever else
// the host creates in between.  An engine returns its stream to the pool when it is destroyed.  HPS_STREAM_POOL=<n> sets the
// pool's size (0 = a fresh stream per engine, as before).  Default 3: with the process's null stream that is the runtime's
// default of 4 hardware queues per priority (GPU_MAX_HW_QUEUES) -- a 4th pooled stream has to share one of those queues,
// and two processes on one device with pools of 4 made 1249 slices/s together against 1916-1928 with pools of 0-3
// (profiles/r05_stream_pool_two_processes.txt).  Further engines get streams of their own.
// Self-check of the engines' stream pool (HPS_STREAM_POOL_CHECK=0: off).  The pool's size is a property of the runtime read
// off one box (four front-end pipes per priority less the null stream's: streams created back to back land on different
// pipes up to 3; a fourth shares one -- profiles/r05_queue_pairs.txt, r05_stream_pool_two_processes.txt).  Another runtime, or
// a process that had created streams of its own first, may map two pool streams to one pipe, and three stages in flight
// then take turns without anything saying so.  So once per device, when the pool is made: a one-workgroup kernel that spins
// for 100 us, R times on both streams of every pair; side by side takes R x 100 us, taking turns 2 R x 100 us.
__global__ void k_pool_spin (long long ticks)
{
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
namespace { std::map<int, int> g_pool_shared_pairs; }
static void check_stream_pool (int device, const std::vector<hipStream_t>& pool)
{
    g_pool_shared_pairs[device] = -1;
    if (const char* v = std::getenv("HPS_STREAM_POOL_CHECK")) if (std::atoi(v) == 0) return;
    if (pool.size() < 2) { g_pool_shared_pairs[device] = 0; return; }
    int rate = 0;
    if (hipDeviceGetAttribute(&rate, hipDeviceAttributeWallClockRate, device) != hipSuccess || rate <= 0) return;
    const long long ticks = (long long)rate/10;                 // (kHz: 100 us)
    const int R = 4;
    int shared = 0;
    std::string which;
    for (size_t i = 0; i < pool.size(); ++i) for (size_t j = i + 1; j < pool.size(); ++j) {
        hipLaunchKernelGGL(k_pool_spin, dim3(1), dim3(64), 0, pool[i], ticks/20);      // (code object loaded, queues awake)
        hipLaunchKernelGGL(k_pool_spin, dim3(1), dim3(64), 0, pool[j], ticks/20);
        (void)hipStreamSynchronize(pool[i]); (void)hipStreamSynchronize(pool[j]);
        const auto t0 = std::chrono::steady_clock::now();
        for (int r = 0; r < R; ++r) {
            hipLaunchKernelGGL(k_pool_spin, dim3(1), dim3(64), 0, pool[i], ticks);
            hipLaunchKernelGGL(k_pool_spin, dim3(1), dim3(64), 0, pool[j], ticks);
        }
        (void)hipStreamSynchronize(pool[i]); (void)hipStreamSynchronize(pool[j]);
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        if (us > 1.6*R*100.0) { ++shared; which += " (" + std::to_string(i) + "," + std::to_string(j) + "): " + std::to_string((int)us) + " us"; }
    }
    g_pool_shared_pairs[device] = shared;
    if (shared)
        std::fprintf(stderr, "libhpslice: device %d: %d pair(s) of the %zu engine streams of the pool take turns instead of running side by side "
                             "(%d x 100 us on both streams of a pair, expected %d us:%s) -- several stages in flight on this device will share a "
                             "front-end pipe; try HPS_STREAM_POOL=%zu or GPU_MAX_HW_QUEUES\n", device, shared, pool.size(), R, R*100, which.c_str(), pool.size() - 1);
}
extern "C" int hps_stream_pool_shared_pairs (int device)      // -1: not checked (no pool yet, or HPS_STREAM_POOL_CHECK=0)
{
    std::lock_guard<std::mutex> lock(g_pool_mutex);
    auto it = g_pool_shared_pairs.find(device);
    return it == g_pool_shared_pairs.end() ? -1 : it->second;
}

hipError_t create_engine_stream (hipStream_t* s, int device, bool* pooled)
{
    *pooled = false;
    const char* v = std::getenv("HPS_CU_MASKS");
    if (!v || !std::strchr(v, '-')) {                       // (unset, or no range in it)
        int want = 3;
        if (const char* p = std::getenv("HPS_STREAM_POOL")) want = std::atoi(p);
        if (want <= 0) return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
        std::lock_guard<std::mutex> lock(g_pool_mutex);
        std::vector<hipStream_t>& pool = g_stream_pool[device];
        if (!g_pool_made[device]) {
            g_pool_made[device] = true;
            void* scratch = nullptr;
            if (hipMalloc(&scratch, 256) != hipSuccess) scratch = nullptr;
            for (int k = 0; k < want; ++k) {
                hipStream_t t = nullptr;
                if (hipStreamCreateWithFlags(&t, hipStreamNonBlocking) != hipSuccess) break;
                // the first command makes the runtime acquire the stream's hardware queue: now, in this order
                if (scratch) { (void)hipMemsetAsync(scratch, 0, 256, t); (void)hipStreamSynchronize(t); }
                pool.push_back(t);
            }
            if (scratch) (void)hipFree(scratch);
            check_stream_pool(device, pool);
            std::reverse(pool.begin(), pool.end());          // (handed out from the back: first created first)
        }
        if (pool.empty()) return hipStreamCreateWithFlags(s, hipStreamNonBlocking);       // more engines than the pool holds
        *s = pool.back(); pool.pop_back(); *pooled = true;
        return hipSuccess;
    }
    static std::atomic<int> created{0};
    std::vector<std::string> entries;
    {   std::string cur; for (const char* p = v; ; ++p) { if (*p == ',' || !*p) { entries.push_back(cur); cur.clear(); if (!*p) break; } else cur += *p; } }
    const std::string& e = entries[created++ % entries.size()];
    uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    size_t pos = 0;
    while (pos < e.size()) {
        size_t end = e.find('+', pos); if (end == std::string::npos) end = e.size();
        int lo = 0, hi = -1;
        if (std::sscanf(e.substr(pos, end - pos).c_str(), "%d-%d", &lo, &hi) == 2)
            for (int b = std::max(lo, 0); b <= std::min(hi, 255); ++b) mask[b >> 5] |= 1u << (b & 31);
        pos = end + 1;
    }
    return hipExtStreamCreateWithCUMask(s, 8, mask);
}

// ~Engine: a pooled stream goes back to its device's pool once its work is done
void return_engine_stream (hipStream_t st, int device)
{
    (void)hipStreamSynchronize(st);
    std::lock_guard<std::mutex> lock(g_pool_mutex);
    g_stream_pool[device].push_back(st);
}

} // namespace hps
