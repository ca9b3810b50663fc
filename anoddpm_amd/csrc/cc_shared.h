// The union-find primitives of the connected-component launches, stated once for the planes of csrc/postproc.hip and the volumes
// of csrc/postproc3d.hip.  Labels are 32-bit words in global memory: label[i] is the index of an element of the same component
// with label[i] <= i, or -1 on the background; a root names itself.  A label never grows and always names an element of the same
// component, so a stale read costs a retry, never a wrong answer; no workgroup waits on another.  Nothing here knows how many
// dimensions the elements are laid out in: only the link launch of each file does (it is the one that names neighbours).
#pragma once
#include "common.h"

namespace anoddpm {
namespace cc {

constexpr int THREADS = 256;

// Every launch: `bps` workgroups per segment (a plane, a volume), thread -> element p of its segment, global index
// seg * n + p < 2^31.
struct Pixel { int64_t plane; int p, idx; bool valid; };

__device__ __forceinline__ Pixel pixel_of(int bps, int n)
{
    Pixel q;
    q.plane = blockIdx.x / bps;
    q.p = (int)(blockIdx.x % bps) * THREADS + (int)threadIdx.x;
    q.valid = q.p < n;
    q.idx = (int)(q.plane * n + q.p);
    return q;
}

__device__ __forceinline__ int load_label(const int *label, int i)
{
    return __hip_atomic_load(label + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int find_root(const int *label, int x)
{
    for (;;) {
        const int p = load_label(label, x);                          // p <= x always: the walk ends
        if (p == x) return x;
        x = p;
    }
}

__device__ inline void link(int *label, int a, int b)
{
    for (;;) {
        a = find_root(label, a);
        b = find_root(label, b);
        if (a == b) return;
        if (a > b) { const int s = a; a = b; b = s; }
        const int old = atomicMin(&label[b], a);
        if (old == b) return;                                        // b was a root and now hangs below a
        b = old;                                                     // b had a parent already: join that one with a as well
    }
}

// size[root] += 1 for every lane whose root is >= 0 (-1: background or past the end): one add per wave for the lanes that share
// the first foreground lane's root, one add each for the others.
__device__ __forceinline__ void add_sizes(int *size, int root)
{
    const bool fg = root >= 0;
    const unsigned long long any = __ballot(fg);
    if (any == 0) return;
    const int leader = __ffsll(any) - 1;
    const int first = __shfl(root, leader);
    const bool same = fg && root == first;
    const unsigned long long group = __ballot(same);
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&size[first], __popcll(group));
    else if (fg && !same) atomicAdd(&size[root], 1);
}

}  // namespace cc
}  // namespace anoddpm
