// Host-side helpers shared by the launchers: a HIP error as a C-ABI return code, the pointer alignment test, the launch helpers, what an
// array-style *_plan export reports, per-device caches (thread-safe), environment knobs read once.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/stego_corr.h"
#include "dispatch.h"
#include "ws_layout.h"

namespace stego {

// what a launcher returns for the runtime's answer to its launch
inline int hip_rc(hipError_t e) { return e == hipSuccess ? STEGO_OK : STEGO_ERR_HIP + (int)e; }

inline bool aligned(const void* ptr, size_t a) { return (reinterpret_cast<uintptr_t>(ptr) % a) == 0; }

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-device property of a kernel: remember what each
// (device, kernel) pair already has, under a mutex (one process may drive several GPUs from several threads, as the
// reference's DataParallel feature extraction does, precompute_knns.py:59).
hipError_t ensure_dynamic_lds(const void* kernel, int bytes);

// One launch of one instantiation: the dynamic-LDS attribute (only when lds > 0), the launch, the runtime's answer to it.  The kernel is
// named once, as the template argument, so the attribute and the launch cannot mean different instantiations.  (allow_dynamic_lds on its
// own, where attribute and launch are not one to one: corr_wide.hip sets two kernels' attributes once, in front of a loop of launches;
// the add-on units launch through launch_first / launch_next below, which set it only beyond the 64 KB that every kernel may use.)
template <auto Kernel>
inline hipError_t allow_dynamic_lds(int lds) { return lds > 0 ? ensure_dynamic_lds(reinterpret_cast<const void*>(Kernel), lds) : hipSuccess; }

template <auto Kernel, class... Args>
inline hipError_t launch(dim3 grid, dim3 block, int lds, hipStream_t stream, const Args&... args)
{
    const hipError_t e = allow_dynamic_lds<Kernel>(lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(Kernel, grid, block, lds, stream, args...);
    return hipGetLastError();
}

// The add-on units' launch (crf_loss, augment, rec_loss, corr_heat, corr_pr, the probe units, salience_draw, optim_step): the attribute
// only beyond the 64 KB of dynamic LDS that every kernel may use, and launch_first clears what an earlier call left in the thread's
// sticky error before it launches, so the answer is this launch's own.  launch_next is for a further launch of the same API call, right
// after a launch that answered hipSuccess: there is nothing to clear.
template <auto Kernel, class... Args>
inline hipError_t launch_next(dim3 grid, dim3 block, size_t lds, hipStream_t stream, const Args&... args)
{
    if (lds > 64 * 1024) {
        const hipError_t e = allow_dynamic_lds<Kernel>((int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds, stream, args...);
    return hipGetLastError();
}

template <auto Kernel, class... Args>
inline hipError_t launch_first(dim3 grid, dim3 block, size_t lds, hipStream_t stream, const Args&... args)
{
    if (lds > 64 * 1024) {
        const hipError_t e = allow_dynamic_lds<Kernel>((int)lds);
        if (e != hipSuccess) return e;
    }
    (void)hipGetLastError();
    hipLaunchKernelGGL(Kernel, grid, block, lds, stream, args...);
    return hipGetLastError();
}

// What an array-style *_plan export answers: the descriptor's return code, and per launch its LDS bytes and workgroups - zeros when the
// descriptor is bad (lds / wgs are not read then).  Either output may be NULL.
inline int report_plan(int rc, int n, const size_t* lds, const int64_t* wgs, size_t* lds_out, int64_t* wgs_out)
{
    for (int i = 0; i < n; ++i) {
        if (lds_out) lds_out[i] = rc == STEGO_OK ? lds[i] : 0;
        if (wgs_out) wgs_out[i] = rc == STEGO_OK ? wgs[i] : 0;
    }
    return rc;
}

// with_const (dispatch.h) for launchers that have no instantiation for an unlisted value
template <int... Vs, class F>
inline hipError_t with_const_strict(int v, F&& f) { return with_const_or<Vs...>(v, hipErrorInvalidValue, static_cast<F&&>(f)); }

// number of compute units of the current device (cached per device)
int device_cu_count();

// Measurement / ablation knobs: STEGO_DEBUG, STEGO_DEBUG_SAMPLE, STEGO_DEBUG_BWD, STEGO_DEBUG_VIT, STEGO_DEBUG_KNN, STEGO_FWD_VARIANT,
// and one deployment knob, STEGO_SHARED_DEVICE (1: other kernels - the collectives of a data-parallel job - run on the device while the
// loss does: the fused forward then launches no phase-1 helper workgroups and so leaves the compute units beyond its tiles free;
// a value > 8 is an explicit number of phase-1 owner workgroups, for measurements: 232 .. 256 time alike, 224 costs ~1 us).
// Read from the environment once, when the library is loaded; stego_debug_set() (C ABI, tools only) overrides them
// afterwards.  The product path never calls getenv.
enum { KNOB_DEBUG = 0, KNOB_DEBUG_SAMPLE, KNOB_DEBUG_BWD, KNOB_DEBUG_VIT, KNOB_DEBUG_KNN, KNOB_FWD_VARIANT, KNOB_SHARED_DEVICE, KNOB_COUNT };
int knob(int which);
void set_knob(int which, int value);

// test hook (stego_debug_occupy): n_wg workgroups of 256 threads with lds_bytes of LDS each spin for `micros`
hipError_t launch_occupy(int n_wg, int lds_bytes, int micros, hipStream_t stream);
// A stream of the library's own per device + a pinned flag word: side_begin() returns the stream (creating both on the first call for a
// device - NOT while a capture is under way), side_finish() returns when everything enqueued on it has run, by watching the flag a
// one-thread kernel sets: no HIP synchronisation API is called, so both are legal while the calling thread captures another stream.
hipError_t side_begin(hipStream_t* stream);
hipError_t side_finish();

}  // namespace stego
