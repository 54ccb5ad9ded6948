// rt_comm.hip — host side of libpathtracer.so: the RCCL exchange of sample buffers
// between ranks.
#include "runtime.hpp"

using namespace ptrt;

extern "C" {

int ptCommGetUniqueId(uint8_t id[128])
{
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    ncclUniqueId u;
    ncclResult_t e = ncclGetUniqueId(&u);
    if (e != ncclSuccess) { SetError("ncclGetUniqueId: %s", ncclGetErrorString(e)); return (int)e; }
    std::memcpy(id, &u, 128);
    return 0;
}

pt_comm* ptCommCreate(pt_device* d, int nranks, int rank, const uint8_t id[128])
{
    if (!d || nranks < 1 || rank < 0 || rank >= nranks) { SetError("bad comm arguments"); return nullptr; }
    if (hipSetDevice(d->id) != hipSuccess) { SetError("hipSetDevice failed"); return nullptr; }
    ncclUniqueId u;
    std::memcpy(&u, id, 128);
    pt_comm* c = new pt_comm;
    c->dev = d;
    c->nranks = nranks;
    c->rank = rank;
    if (hipMalloc(&c->flag, sizeof(int)) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&c->host_flag), sizeof(int), hipHostMallocDefault) != hipSuccess) {
        SetError("comm flag allocation failed");
        if (c->flag) (void)hipFree(c->flag);
        delete c;
        return nullptr;
    }
    ncclResult_t e = ncclCommInitRank(&c->comm, nranks, u, rank);
    if (e != ncclSuccess) {
        SetError("ncclCommInitRank: %s", ncclGetErrorString(e));
        (void)hipFree(c->flag);
        (void)hipHostFree(c->host_flag);
        delete c;
        return nullptr;
    }
    d->comms.push_back(c);
    return c;
}

void ptCommDestroy(pt_comm* c)
{
    if (!c) return;
    if (pt_device* d = c->dev) {
        (void)hipSetDevice(d->id);
        auto& v = d->comms;
        v.erase(std::remove(v.begin(), v.end(), c), v.end());
        // A CommAgree readback left queued by a wait that failed (which
        // aborted the communicator) lands before the pinned word is freed:
        // the abort stops RCCL's kernels, and after an abort a wait gives up
        // within 10 s.
        if (c->aborted) (void)DeviceWait(d);
    }
    if (c->comm) (void)ncclCommDestroy(c->comm);
    if (c->flag) (void)hipFree(c->flag);
    if (c->host_flag) (void)hipHostFree(c->host_flag);
    delete c;
}

int ptCommSetTimeout(pt_comm* c, double seconds)
{
    if (!c || !(seconds > 0.0)) { SetError("ptCommSetTimeout: bad argument"); return -1; }
    c->timeout_s = seconds;
    return 0;
}

namespace {

int CommUsable(pt_device* d, pt_comm* c)
{
    if (!d || !c) { SetError("null argument"); return -1; }
    if (!c->dev) { SetError("communicator's device was destroyed"); return -1; }
    if (c->aborted || !c->comm) {
        SetError("communicator aborted after an earlier failure (rank %d of %d)", c->rank, c->nranks);
        return PT_ERROR_COMM_ABORTED;
    }
    if (c->dev != d) { SetError("communicator belongs to another device"); return -1; }
    return 0;
}

// A collective was just enqueued: its synchronous result and the
// communicator's asynchronous error state (non-blocking).  Any failure aborts
// the device's communicators, so no rank is left inside a collective whose
// peers have given up.
int CommEnqueued(pt_device* d, pt_comm* c, ncclResult_t e, const char* what)
{
    ncclResult_t st = ncclSuccess;
    if (e == ncclSuccess && ncclCommGetAsyncError(c->comm, &st) == ncclSuccess && (st == ncclSuccess || st == ncclInProgress))
        return 0;
    SetError("%s: %s; communicators aborted", what, ncclGetErrorString(e != ncclSuccess ? e : st));
    AbortComms(d);
    return PT_ERROR_COMM_ABORTED;
}

// Collective agreement on the caller's argument checks before a collective:
// every rank contributes `bad` (non-zero = its check failed) to a one-word
// max all-reduce and waits for it, so either every rank enters the
// collective or none does (a check failing on one rank only would otherwise
// leave the others blocked inside it).  Returns 0 when every rank passed.
int CommAgree(pt_device* d, pt_comm* c, int bad, const char* what)
{
    if (c->nranks == 1) return bad ? -1 : 0;
    // Pinned host word both ways: the copies are truly asynchronous, so a
    // hung peer is seen by DeviceWait's polling (a pageable copy would block
    // inside hipMemcpyAsync), and a readback still queued when the wait gives
    // up writes into memory that lives until ptCommDestroy.
    *c->host_flag = bad ? 1 : 0;
    PT_HIP(hipMemcpyAsync(c->flag, c->host_flag, sizeof(int), hipMemcpyHostToDevice, d->stream));
    ncclResult_t e = ncclAllReduce(c->flag, c->flag, 1, ncclInt32, ncclMax, c->comm, d->stream);
    if (int r = CommEnqueued(d, c, e, what)) return r;
    PT_HIP(hipMemcpyAsync(c->host_flag, c->flag, sizeof(int), hipMemcpyDeviceToHost, d->stream));
    PT_WAIT(d);
    const int h = *c->host_flag;
    if (h && !bad) {
        SetError("%s: the arguments failed their check on another rank; nothing was exchanged", what);
        return -1;
    }
    return h ? -1 : 0;
}

}  // namespace

int ptCommReduceSampleBuffer(pt_device* d, pt_comm* c, pt_sample_buffer* b, int root)
{
    if (int e = CommUsable(d, c)) return e;
    PT_HIP(hipSetDevice(d->id));
    // Argument checks, agreed on by every rank (CommAgree).  The rows zeroed
    // below are those outside the buffer's partition, so the partition must
    // be this communicator's rank of nranks.  A whole-frame buffer on a
    // multi-rank communicator is a sample shard: reducing it in place would
    // add the root's previous totals again on a repeated call.  (A one-rank
    // communicator sums nothing across ranks; it may reduce any partition --
    // the zeroing alone is then observable.)
    int bad = 0;
    if (!b) { SetError("null sample buffer"); bad = 1; }
    else if (root < 0 || root >= c->nranks) { SetError("bad root %d", root); bad = 1; }
    else if (b->nranks == 1 && c->nranks > 1) {
        SetError("ptCommReduceSampleBuffer: whole-frame buffer on a %d-rank communicator (sample shards: use "
                 "ptCommReduceSampleBufferInto)", c->nranks);
        bad = 1;
    } else if (c->nranks > 1 && b->nranks > 1 && ((int)b->nranks != c->nranks || (int)b->rank != c->rank)) {
        SetError("sample buffer partition %u/%u does not match communicator rank %d of %d", b->rank, b->nranks,
                 c->rank, c->nranks);
        bad = 1;
    }
    if (int e = CommAgree(d, c, bad, "ptCommReduceSampleBuffer")) return e;
    size_t count = (size_t)b->width * b->height * 4;
    // Only the bands this rank renders may enter the sum: at the root the
    // other rows hold the previous reduce's totals (a progressive frame
    // reduces again after more rounds), so they are zeroed first and the
    // in-place sum stays exact on every call.
    PT_HIP(pt_launch_zero_unowned(b->accum, b->width, b->height, b->rank, b->nranks, d->stream));
    ncclResult_t e = ncclReduce(b->accum, b->accum, count, ncclFloat32, ncclSum, root, c->comm, d->stream);
    return CommEnqueued(d, c, e, "ncclReduce");
}

int ptCommReduceSampleBufferInto(pt_device* d, pt_comm* c, pt_sample_buffer* b, pt_sample_buffer* total, int root)
{
    if (int e = CommUsable(d, c)) return e;
    PT_HIP(hipSetDevice(d->id));
    const bool is_root = c->rank == root;
    int bad = 0;
    if (!b) { SetError("null sample buffer"); bad = 1; }
    else if (root < 0 || root >= c->nranks) { SetError("bad root %d", root); bad = 1; }
    else if (is_root && (!total || total->width != b->width || total->height != b->height)) {
        SetError("ptCommReduceSampleBufferInto: the root needs a total buffer of the same size");
        bad = 1;
    }
    if (int e = CommAgree(d, c, bad, "ptCommReduceSampleBufferInto")) return e;
    size_t count = (size_t)b->width * b->height * 4;
    ncclResult_t e = ncclReduce(b->accum, is_root ? total->accum : b->accum, count, ncclFloat32, ncclSum, root, c->comm,
                                d->stream);
    return CommEnqueued(d, c, e, "ncclReduce");
}

// The same frame-end exchange with 1/N of the traffic: the bands are
// disjoint, so the root needs only each band's owner's rows.  Band b (rows
// [16b, 16b+16), contiguous in the row-major buffer) is owned by rank
// b % nranks; every non-root owner sends its bands to the root, which
// receives them in place.  One group of point-to-point transfers: each peer
// pushes ~1/N of the frame over its own xGMI link to the root concurrently,
// instead of a ring reduction of the whole buffer.
int ptCommGatherSampleBuffer(pt_device* d, pt_comm* c, pt_sample_buffer* b, int root)
{
    if (int e = CommUsable(d, c)) return e;
    PT_HIP(hipSetDevice(d->id));
    int bad = 0;
    if (!b) { SetError("null sample buffer"); bad = 1; }
    else if (root < 0 || root >= c->nranks) { SetError("bad root %d", root); bad = 1; }
    else if ((int)b->nranks != c->nranks || (int)b->rank != c->rank) {
        SetError("sample buffer partition %u/%u does not match communicator rank %d of %d", b->rank, b->nranks,
                 c->rank, c->nranks);
        bad = 1;
    }
    if (int e = CommAgree(d, c, bad, "ptCommGatherSampleBuffer")) return e;
    if (c->nranks == 1) return 0;
    uint32_t bands = (b->height + 15) / 16;
    ncclResult_t e = ncclGroupStart();
    for (uint32_t band = 0; band < bands && e == ncclSuccess; band++) {
        int owner = (int)(band % (uint32_t)c->nranks);
        if (owner == root) continue;
        uint32_t rows = std::min<uint32_t>(16u, b->height - band * 16u);
        float* p = reinterpret_cast<float*>(b->accum + (size_t)band * 16 * b->width);
        size_t count = (size_t)rows * b->width * 4;
        if (c->rank == owner) e = ncclSend(p, count, ncclFloat32, root, c->comm, d->stream);
        else if (c->rank == root) e = ncclRecv(p, count, ncclFloat32, owner, c->comm, d->stream);
    }
    ncclResult_t g = ncclGroupEnd();
    if (e == ncclSuccess) e = g;
    return CommEnqueued(d, c, e, "band gather");
}

}  // extern "C"
