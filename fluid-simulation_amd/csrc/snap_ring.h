// The two-slot hand-off every kind of snapshot uses (density leaves: fluid_output.hip, level set: fluid_sdf.hip, mesh: fluid_mesh.hip).
//
// A snapshot's kernels write its records into a slot's device staging on the handle's stream; the records then travel to the
// slot's pinned buffer in one copy on a second, non-blocking stream behind an event, while the handle's stream is free for the
// next fluid_step.  Snapshot q lives in slot q & 1, so a slot is written by snapshot q, q + 2, ...: what a wait handed out stays
// valid until the second following snapshot of the same kind.  At most two snapshots are outstanding (taken and not yet waited
// for): a third is refused before anything is launched, and a refused or failed snapshot is not outstanding, because n_snap moves
// only in snap_commit.  What a kind has to remember per snapshot beside the bytes (counts, constants) it keeps in two-element
// arrays of its own, indexed by the same parity.  Each kind has a ring of its own: all of them can be taken in one step.
//
// Included by sim.h (HIPCHK); everything is inline.
#pragma once

struct SnapSlot {
    char* dev = nullptr;         // device staging
    char* host = nullptr;        // pinned
    size_t cap = 0;              // bytes either buffer holds
    hipEvent_t done = nullptr;   // recorded on the copy stream behind the slot's copy
};
struct SnapRing {
    hipStream_t copy = nullptr;
    hipEvent_t ready = nullptr;    // recorded on the handle's stream behind the kernels that fill the staging
    SnapSlot s[2];
    long n_snap = 0, n_wait = 0;   // snapshots taken / waited for
};

inline int snap_init(SnapRing& r)
{
    HIPCHK(hipStreamCreateWithFlags(&r.copy, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&r.ready, hipEventDisableTiming));
    for (SnapSlot& q : r.s) HIPCHK(hipEventCreateWithFlags(&q.done, hipEventDisableTiming));
    return FLUID_OK;
}

// waits for the copies in flight, then frees whatever snap_init and snap_reserve got
inline void snap_free(SnapRing& r)
{
    if (r.copy) hipStreamSynchronize(r.copy);
    for (SnapSlot& q : r.s) {
        if (q.dev) hipFree(q.dev);
        if (q.host) hipHostFree(q.host);
        if (q.done) hipEventDestroy(q.done);
    }
    if (r.ready) hipEventDestroy(r.ready);
    if (r.copy) hipStreamDestroy(r.copy);
    r = SnapRing{};
}

inline bool snap_full(const SnapRing& r) { return r.n_snap - r.n_wait >= 2; }   // the next snapshot would be the third outstanding
inline int snap_slot(const SnapRing& r) { return (int)(r.n_snap & 1); }         // where the next snapshot goes

// room for `bytes` in the slot (its earlier contents were handed out two snapshots ago: no longer promised)
inline int snap_reserve(SnapSlot& q, size_t bytes, size_t slack)
{
    if (bytes <= q.cap) return FLUID_OK;
    if (q.dev) hipFree(q.dev);
    if (q.host) hipHostFree(q.host);
    q.dev = q.host = nullptr;
    q.cap = 0;
    const size_t cap = bytes + bytes / 2 + slack;
    HIPCHK(hipMalloc((void**)&q.dev, cap));
    HIPCHK(hipHostMalloc((void**)&q.host, cap));
    q.cap = cap;
    return FLUID_OK;
}

// the kernels queued on `st` have filled the first `bytes` of the next slot's staging: send them to its pinned buffer.  An empty
// snapshot (bytes == 0) copies nothing and is outstanding all the same.
inline int snap_commit(SnapRing& r, hipStream_t st, size_t bytes)
{
    SnapSlot& q = r.s[snap_slot(r)];
    if (bytes > 0) {
        HIPCHK(hipEventRecord(r.ready, st));
        HIPCHK(hipStreamWaitEvent(r.copy, r.ready, 0));
        HIPCHK(hipMemcpyAsync(q.host, q.dev, bytes, hipMemcpyDeviceToHost, r.copy));
    }
    HIPCHK(hipEventRecord(q.done, r.copy));
    r.n_snap++;
    return FLUID_OK;
}

// *k = the slot of the oldest outstanding snapshot, its copy waited for and the snapshot no longer outstanding; -1: there is none
inline int snap_next_wait(SnapRing& r, int* k)
{
    *k = -1;
    if (r.n_wait >= r.n_snap) return FLUID_OK;
    HIPCHK(hipEventSynchronize(r.s[r.n_wait & 1].done));
    *k = (int)(r.n_wait++ & 1);
    return FLUID_OK;
}
