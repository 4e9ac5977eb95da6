// pbre_sidepick.hpp -- choosing a side stream that really runs beside the caller's stream.
//
// HIP multiplexes streams onto a few hardware queues (4 by default); two streams that share one do not overlap -- their kernels run in
// submission order -- and which streams share is an accident of the process's stream-creation history.  Measured in bench.py's process
// (iCub pipeline, 32768 envs): 0.62 ms per step with the side stream on the caller's queue, 0.35 ms on another one, 0.40 ms without any
// side stream.  So an engine keeps a few candidate streams and, once per caller stream, times two 150 us busy-wait kernels -- one on the
// caller's stream, one on a candidate, forked and joined with the events the step itself uses: the first candidate that overlaps wins.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include "pbre_devmem.hpp"

namespace pbre {

static __global__ void k_spin_ticks(long long ticks) {       // busy-wait for `ticks` of the 100 MHz wall clock
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

struct SidePick {
    static constexpr int NCAND = 4;
    Stream cand[NCAND];
    hipStream_t side = nullptr;
    struct { hipStream_t s, side; } cache[4] = {};      // picks made so far (caller stream -> side stream), round robin
    int ncache = 0;
    Event t0, t1, fork, join;
    int probes = 0;                    // calibration runs so far (diagnostics)
    ~SidePick() { for (auto& c : cand) if (c) (void)hipStreamSynchronize(c); }      // every candidate idle before it -- and what its kernels use -- is released
    hipError_t create(int priority, bool with_priority) {
        hipError_t e;
        for (auto& c : cand) {
            e = with_priority ? hipStreamCreateWithPriority(c.out(), hipStreamNonBlocking, priority) : hipStreamCreateWithFlags(c.out(), hipStreamNonBlocking);
            if (e != hipSuccess) return e;
        }
        side = cand[0];
        if ((e = hipEventCreate(t0.out())) != hipSuccess) return e;
        if ((e = hipEventCreate(t1.out())) != hipSuccess) return e;
        if ((e = hipEventCreateWithFlags(fork.out(), hipEventDisableTiming)) != hipSuccess) return e;
        return hipEventCreateWithFlags(join.out(), hipEventDisableTiming);
    }
    // the side stream to use beside caller stream s (synchronises s the first time it sees it; PBRE_SIDE_PROBE=0: no calibration)
    hipStream_t pick(hipStream_t s) {
        if (!cand[0]) return side;
        for (int k = 0; k < (ncache < 4 ? ncache : 4); k++) if (cache[k].s == s) return side = cache[k].side;
        side = pick_new(s);
        cache[ncache % 4].s = s; cache[ncache % 4].side = side; ncache++;
        return side;
    }
    hipStream_t pick_new(hipStream_t s) {
        side = cand[0];
        const char* knob = getenv("PBRE_SIDE_PROBE");
        if (knob && knob[0] == '0') return side;
        // (round-2 advice) the probe launches busy-wait kernels and waits for an event on the host: never on a stream that is being
        // captured into a graph (it would invalidate the capture) -- such a caller gets the first candidate, uncalibrated
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (s && hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) return side;
        (void)hipGetLastError();
        probes++;
        for (int k = 0; k < NCAND; k++) {
            (void)hipEventRecord(t0, s);
            (void)hipEventRecord(fork, s); (void)hipStreamWaitEvent(cand[k], fork, 0);
            hipLaunchKernelGGL(k_spin_ticks, dim3(1), dim3(64), 0, cand[k], 15000LL);
            (void)hipEventRecord(join, cand[k]);
            hipLaunchKernelGGL(k_spin_ticks, dim3(1), dim3(64), 0, s, 15000LL);
            (void)hipStreamWaitEvent(s, join, 0);
            (void)hipEventRecord(t1, s);
            float ms = 1e9f;
            if (hipEventSynchronize(t1) != hipSuccess || hipEventElapsedTime(&ms, t0, t1) != hipSuccess) break;
            if (getenv("PBRE_SIDE_DEBUG")) fprintf(stderr, "[pbre] side-stream probe: caller %p candidate %d: %.3f ms\n", (void*)s, k, ms);
            if (ms < 0.24f) { side = cand[k]; break; }
        }
        (void)hipGetLastError();
        return side;
    }
};

}  // namespace pbre
