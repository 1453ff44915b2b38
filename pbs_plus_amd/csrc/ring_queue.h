// The page ring's queue protocol on the device: the SHA-256 services (kernels.hip) take chunks from the queues and drop
// page references, the cut side (k_ring_control, ring_kernels.hip) fills the queues and drops the open chunks' holds.
#pragma once

#include "kernel_util.h"
#include "kernels.h"

namespace pbsk {

// ---- the queue protocol the services share with the cut side (k_ring_control) and the host (ring.cpp) --------------------
// Every helper is called with the same arguments in every lane of a wave (per-lane values go in as predicates).
// * Queue words are read RELAXED at device scope: a poll must not invalidate the cache. Only a lane that goes on to read
//   what a position holds pays ONE acquire fence, behind which the descriptor and the chunk's bytes (written by other
//   kernels while the service runs) are visible; the cut side publishes a tail with release.
// * A page reference is dropped with RELEASE once the chunk's last block is in registers: every load of the chunk has
//   completed before the page can go back to the host and be refilled.
// * The record cell's flag and the free-page FIFO live in mapped pinned memory the host polls: system scope, and the
//   digest is fenced out (system) before its flag.

// rank of this lane among the lanes of m
__device__ __forceinline__ uint32_t wave_rank(const unsigned long long m, const int lane) {
    return (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// batch queue: the wave's leader claims n positions with one atomicAdd; the first of them, in every lane
__device__ __forceinline__ uint32_t wave_claim(uint32_t *queue, const unsigned long long m, const uint32_t n, const int lane) {
    uint32_t first = 0;
    const int leader = __ffsll((long long)m) - 1;
    if (lane == leader) first = atomicAdd(queue, n);
    return __shfl(first, leader, 64);
}

// published, not yet taken positions of a compare-and-swap queue word {tail, head} (RingCtl::lq, sq), and its head
__device__ __forceinline__ int32_t ring_queue_avail(const unsigned long long *q, uint32_t &head) {
    const unsigned long long v = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    head = (uint32_t)(v >> 32);
    return (int32_t)((uint32_t)v - head);
}

// Compare-and-swap claim on such a queue: the leader of the lanes in m moves `head` from h to h + cnt, and only over published
// positions (0 < cnt <= what ring_queue_avail saw), so no lane ever waits at a position of this queue. Returns the first position
// claimed, in every lane; ~0u when another wave moved `head` first (nothing claimed: look again next time). The lane of rank i
// in m (i < cnt) owns position first + i. (`h` by reference: as a by-value argument it would tell the optimiser that the
// queue word is never undef, which drops a freeze and moves the pair service's long-queue test from scalar to vector code.)
__device__ __forceinline__ uint32_t ring_cas_claim(uint32_t *head, const uint32_t &h, const uint32_t cnt, const unsigned long long m,
                                                   const int lane) {
    const int leader = __ffsll((long long)m) - 1;
    uint32_t first = 0xffffffffu;
    if (lane == leader && atomicCAS(head, h, h + cnt) == h) first = h;
    first = __shfl(first, leader, 64);
    if (first != 0xffffffffu) __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return first;
}

// the descriptor at queue slot `slot`, loaded by the lanes of `pred` only (zero elsewhere)
__device__ __forceinline__ void ring_desc_load(const uint4 *q, const uint32_t slot, const bool pred, uint4 &e0, uint4 &e1) {
    e0 = make_uint4(0, 0, 0, 0);
    e1 = make_uint4(0, 0, 0, 0);
    if (pred) {
        e0 = q[2u * slot];
        e1 = q[2u * slot + 1u];
    }
}

// lanes of `take` make the descriptor their chunk: both piece addresses, length, first-piece length, digest destination in
// the record cell, page references. (Selects, not conditional stores: two flags set in sibling branches get their stores
// merged through a selected pointer by the optimiser, which moves both into scratch memory.)
__device__ __forceinline__ void ring_desc_take(const RingSource &src, const bool take, const uint4 e0, const uint4 e1,
                                               const uint8_t *&base, const uint8_t *&base2, uint64_t &len, uint32_t &len1,
                                               uint8_t *&dst, uint32_t &pages) {
    const RingDesc d = ring_desc_decode(e0, e1);
    base = take ? reinterpret_cast<const uint8_t *>(d.p1) : base;
    base2 = take ? reinterpret_cast<const uint8_t *>(d.p2v) : base2;
    len = take ? (uint64_t)d.len : len;
    len1 = take ? d.len1 : len1;
    dst = take ? src.cells + (uint64_t)d.cell * kCellBytes + 4u * kCellDigest : dst;
    pages = take ? d.pages : pages;
}

// `stop` is raised (release) behind the last publish of every queue. Once a lane has seen it (relaxed), the queue word q is
// looked at once more behind an acquire fence: true = q is empty as well, the lane may leave. No lane leaves while positions
// are unclaimed.
__device__ __forceinline__ bool ring_drained_after_stop(const unsigned long long *q) {
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    uint32_t h;
    return ring_queue_avail(q, h) <= 0;
}
__device__ __forceinline__ bool ring_stop_raised(const RingSource &src) {
    return (uint32_t)(__hip_atomic_load(&src.ctl->tail_stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 32) != 0u;
}

// a page has no reference left: hand it to the host through the free FIFO ((sequence << 32) | page)
__device__ __forceinline__ void ring_report_free(const RingSource &q, const uint32_t page) {
    const uint32_t fs = atomicAdd(&q.ctl->free_count, 1u);
    __hip_atomic_store(&q.free_fifo[fs & q.free_mask], ((unsigned long long)(fs + 1u) << 32) | page, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}
// drop one reference on a page; whoever brings it to zero reports it free
__device__ __forceinline__ void ring_release_page(const RingSource &q, const uint32_t page) {
    if (__hip_atomic_fetch_sub(&q.pending[page], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT) == 1u) ring_report_free(q, page);
}
// ... the references of a chunk (RingDesc::pages)
__device__ __forceinline__ void ring_release_pages(const RingSource &q, const uint32_t pages) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t pi = h ? (pages >> 16) : (pages & 0xffffu);
        if (pi != 0xffffu) ring_release_page(q, pi);
    }
}

// the digest is in the record cell (dst = its digest words): raise the cell's flag behind it
__device__ __forceinline__ void ring_cell_publish(PBSK_GLOBAL uint32_t *dst) {
    __threadfence_system();
    __hip_atomic_store(dst + (kCellFlag - kCellDigest), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace pbsk
