// rt_device.hip — host side of libpathtracer.so: the error state, the device and its
// stream, the device wait and the launch timing (declared in runtime.hpp).
#include "runtime.hpp"

#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <thread>

namespace {
thread_local std::string g_last_error;
}  // namespace

namespace ptrt __attribute__((visibility("hidden"))) {

void SetError(const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

void AbortComms(pt_device* dev)
{
    for (pt_comm* c : dev->comms) {
        if (c->comm) (void)ncclCommAbort(c->comm);
        c->comm = nullptr;
        c->aborted = true;
    }
    dev->comms.clear();
    dev->comm_failed = true;
}

int DeviceWait(pt_device* dev)
{
    if (dev->comms.empty() && !dev->comm_failed) {
        PT_HIP(hipStreamSynchronize(dev->stream));
        return 0;
    }
    double limit = dev->comm_failed ? 10.0 : 1e30;
    for (pt_comm* c : dev->comms) limit = std::min(limit, c->timeout_s);
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spin = 0;; spin++) {
        hipError_t q = hipStreamQuery(dev->stream);
        if (q == hipSuccess) {
            if (dev->comms.empty()) dev->comm_failed = false;   // drained since the abort
            return 0;
        }
        if (q != hipErrorNotReady) {
            SetError("device stream: %s", hipGetErrorString(q));
            return (int)q;
        }
        for (pt_comm* c : dev->comms) {
            ncclResult_t st = ncclSuccess;
            ncclResult_t r = ncclCommGetAsyncError(c->comm, &st);
            if (r != ncclSuccess || (st != ncclSuccess && st != ncclInProgress)) {
                SetError("RCCL communicator (rank %d of %d) failed: %s; communicators aborted", c->rank, c->nranks,
                         ncclGetErrorString(r != ncclSuccess ? r : st));
                AbortComms(dev);
                return PT_ERROR_COMM_ABORTED;
            }
        }
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (el > limit) {
            SetError("device stream not idle after %.1f s with a live communicator (a peer rank failed or stalled); "
                     "communicators aborted", el);
            AbortComms(dev);
            return PT_ERROR_TIMEOUT;
        }
        if (spin > 64) std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

int BeginTimed(pt_device* dev, int kernel, event_pair& ep, bool sampled, uint32_t rounds)
{
    ep.kernel = -1;
    if (!dev->profiling || !sampled) return 0;
    if (!dev->free_events.empty()) { ep = dev->free_events.back(); dev->free_events.pop_back(); }
    else {
        PT_HIP(hipEventCreate(&ep.a));
        PT_HIP(hipEventCreate(&ep.b));
    }
    ep.kernel = kernel;
    ep.rounds = rounds;
    ep.stream = dev->stream;
    PT_HIP(hipEventRecord(ep.a, ep.stream));
    return 0;
}

int EndTimed(pt_device* dev, event_pair& ep)
{
    if (!dev->profiling || ep.kernel < 0) return 0;
    PT_HIP(hipEventRecord(ep.b, ep.stream));
    dev->pending.push_back(ep);
    return 0;
}

int CollectTimes(pt_device* dev)
{
    if (dev->pending.empty()) return 0;
    PT_WAIT(dev);
    for (event_pair& ep : dev->pending) {
        float ms = 0;
        PT_HIP(hipEventElapsedTime(&ms, ep.a, ep.b));
        dev->launches[ep.kernel] += 1;
        dev->rounds[ep.kernel] += ep.rounds;
        dev->total_ms[ep.kernel] += ms;
        dev->free_events.push_back(ep);
    }
    dev->pending.clear();
    return 0;
}

}  // namespace ptrt

using namespace ptrt;

extern "C" {

const char* ptGetLastError(void) { return g_last_error.c_str(); }

int ptGetDeviceCount(int* count)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    *count = n;
    return 0;
}

pt_device* ptCreateDevice(int hip_device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) { SetError("no HIP device available"); return nullptr; }
    if (hip_device < 0 || hip_device >= n) { SetError("device %d out of range (%d devices)", hip_device, n); return nullptr; }
    if (hipSetDevice(hip_device) != hipSuccess) { SetError("hipSetDevice(%d) failed", hip_device); return nullptr; }
    pt_device* d = new pt_device;
    d->id = hip_device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, hip_device) == hipSuccess && prop.multiProcessorCount > 0)
        d->cu_count = (uint32_t)prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) {
        SetError("device stream creation failed");
        if (d->stream) (void)hipStreamDestroy(d->stream);
        delete d;
        return nullptr;
    }
    return d;
}

void ptDestroyDevice(pt_device* d)
{
    if (!d) return;
    (void)hipSetDevice(d->id);
    (void)DeviceWait(d);
    // Communicators outliving their device: detached (ptCommDestroy still
    // releases them; every exchange on them fails).
    for (pt_comm* c : d->comms) c->dev = nullptr;
    d->comms.clear();
    for (auto& ep : d->pending) { (void)hipEventDestroy(ep.a); (void)hipEventDestroy(ep.b); }
    for (auto& ep : d->free_events) { (void)hipEventDestroy(ep.a); (void)hipEventDestroy(ep.b); }
    for (uint32_t g = 0; g + 1 < PT_MAX_SPLIT; g++) {
        if (d->group_stream[g]) (void)hipStreamDestroy(d->group_stream[g]);
        if (d->join_event[g]) (void)hipEventDestroy(d->join_event[g]);
    }
    if (d->fork_event) (void)hipEventDestroy(d->fork_event);
    if (d->motion_host) (void)hipHostFree(d->motion_host);
    if (d->motion_copied) (void)hipEventDestroy(d->motion_copied);
    (void)hipStreamDestroy(d->stream);
    delete d;
}

int ptSynchronize(pt_device* d)
{
    if (!d) { SetError("null device"); return -1; }
    PT_HIP(hipSetDevice(d->id));
    PT_WAIT(d);
    return 0;
}

int ptSetProfiling(pt_device* d, int enable)
{
    if (!d) { SetError("null device"); return -1; }
    if (int e = CollectTimes(d)) return e;
    d->profiling = enable != 0;
    return 0;
}

int ptSetProfilingPeriod(pt_device* d, uint32_t period)
{
    if (!d || period == 0) { SetError("bad argument"); return -1; }
    d->profile_period = period;
    d->run_tick = 0;
    return 0;
}

int ptGetKernelStats(pt_device* d, int kernel, uint64_t* launches, double* total_ms)
{
    if (!d || kernel < 0 || kernel >= PT_KERNEL_COUNT) { SetError("bad argument"); return -1; }
    PT_HIP(hipSetDevice(d->id));
    if (int e = CollectTimes(d)) return e;
    if (launches) *launches = d->launches[kernel];
    if (total_ms) *total_ms = d->total_ms[kernel];
    return 0;
}

int ptGetKernelRounds(pt_device* d, int kernel, uint64_t* rounds)
{
    if (!d || !rounds || kernel < 0 || kernel >= PT_KERNEL_COUNT) { SetError("bad argument"); return -1; }
    PT_HIP(hipSetDevice(d->id));
    if (int e = CollectTimes(d)) return e;
    *rounds = d->rounds[kernel];
    return 0;
}

int ptResetKernelStats(pt_device* d)
{
    if (!d) { SetError("null device"); return -1; }
    if (int e = CollectTimes(d)) return e;
    for (int k = 0; k < PT_KERNEL_COUNT; k++) { d->launches[k] = 0; d->rounds[k] = 0; d->total_ms[k] = 0; }
    return 0;
}

}  // extern "C"
