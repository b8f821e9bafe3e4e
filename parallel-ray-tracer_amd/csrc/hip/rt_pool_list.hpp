// rt_pool_list.hpp — the indexing of the shadow pool's per-tile job list (rt_shpool.hpp shadow_pool<.., LIST>), kept
// free of HIP so that tests/c/pool_handout_test.cpp can check it with g++ alone against a transcription of the cursor
// hand-out it replaces; the kernel calls the same functions.
//
// A wave's pool holds one job per (owner lane, level, light) whose light passed the back-face test. The cursor
// hand-out visits the groups (level, light) in the order level 0 light 0, level 0 light 1, ..., level 1 light 0, ...,
// hands the owners of a group out in lane order, and gives the k-th idle lane (in lane order) of a refill the k-th job
// not handed out yet. The list is that order written down once per tile: group g's jobs start at base(g) = the number
// of jobs of the groups before it, an owner's slot is base(g) + its rank among the group's owners, and a refill takes
// the slots head .. head + (idle lanes) - 1. Same jobs, same lanes, no loop.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTP_HD __host__ __device__ __forceinline__
#else
#define RTP_HD inline
#endif

namespace rtp {

// a job: owner lane (6 bits) | level << 6 (3 bits: at most 8 levels) | light << 9 (7 bits: the pool's <= 32 lights)
using job_t = std::uint16_t;
RTP_HD job_t job_of(unsigned lane, unsigned level, unsigned light) {
    return (job_t)(lane | (level << 6) | (light << 9));
}
RTP_HD unsigned job_lane(unsigned job) { return job & 63u; }
RTP_HD unsigned job_level(unsigned job) { return (job >> 6) & 7u; }
RTP_HD unsigned job_light(unsigned job) { return job >> 9; }
RTP_HD unsigned job_slot_of_owner(unsigned job) { return job & 511u; }  // 64 level + owner: the path-buffer slot

// the list's words (ints) per wave: 64 lanes x levels x lights jobs of 2 bytes
RTP_HD int list_words(int levels, int lights) { return 32 * levels * lights; }

RTP_HD unsigned popc64(unsigned long long m) { return (unsigned)__builtin_popcountll(m); }
// set bits of m below bit `lane` (the device's mbcnt)
RTP_HD unsigned rank_below(unsigned long long m, unsigned lane) { return popc64(m & ((1ull << lane) - 1ull)); }

// base of the group after one with owner mask m (the running sum the list's builder carries)
RTP_HD unsigned next_base(unsigned base, unsigned long long m) { return base + popc64(m); }
// an owner's slot: its group's base plus its rank among the group's owners
RTP_HD unsigned owner_slot(unsigned base, unsigned rank) { return base + rank; }

// A refill with `head` jobs of `total` handed out: the idle lane of rank k (among the idle lanes, lane order) takes
// slot head + k if that is a job, and the head moves past the jobs taken.
RTP_HD bool take(unsigned head, unsigned total, unsigned k, unsigned& slot) {
    slot = head + k;
    return slot < total;
}
RTP_HD unsigned head_after(unsigned head, unsigned total, unsigned n_idle) {
    const unsigned left = total - head;
    return head + (n_idle < left ? n_idle : left);
}

}  // namespace rtp
