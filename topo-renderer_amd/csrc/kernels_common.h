// kernels_common.h -- what the kernels of every phase share (topo_kernels.hip includes the phase files, in order, into its one
// translation unit).
//
//   the visibility buffer   Vis, view_vis, vis_min / vis_min_unmarked: the frame is a visibility-buffer renderer: every surviving
//                           fragment does a 64-bit atomic min of (depth bits << 32 | draw-order id) -- the minimum reproduces
//                           CompareFunction::Less *and* the API-order tie-break of the reference's in-order draws -- and one resolve
//                           pass shades the winner of each pixel and applies the contour post pass
//   the check build         TOPO_CHK / bounds_violation (-DTOPO_BOUNDS_CHECK)
//   wave helpers            the wave-private LDS fence, wave-uniform values, lane shifts, the constant address space
//
// Integer/float work without a contraction: no MFMA.  Compiled with -ffp-contract=off: results must match the arithmetic spec bit
// for bit.
#pragma once

#include "topo_kernels.h"

namespace topo {
namespace {

// A fragment meets the visibility buffer through one 64-bit atomic min, issued blind: the atomic returns nothing,
// so the wave never waits for it, whereas reading the current key first (to skip fragments that cannot win) puts a
// full memory round trip into every loop that emits fragments.  Measured on c4: k_raster 0.187 -> 0.158 ms,
// k_raster_big 0.45 -> 0.37 ms without the pre-test (profiles/README.md).
// The buffer is tracked in segments of 64 consecutive keys: whoever writes a key marks its segment (a plain byte
// store of 1: racing writers agree), k_clear re-initialises only marked segments, and k_resolve does not even read
// the keys of a block whose segments are all unmarked.  About half of a panorama is sky that no fragment touches.
struct Vis {
    uint64_t* p;             // this view's keys
    const uint64_t* base;    // the whole buffer (segment numbers are global)
    uint8_t* dirty;
#ifdef TOPO_BOUNDS_CHECK
    uint32_t* counters;
    size_t view_keys;        // W * H
#endif
};

// TOPO_BOUNDS_CHECK build (libtopo_hip_check.so, `make check`): every index the kernels form into the visibility buffer,
// the segment marks, the queues, the tile rasters and the outputs is tested first; a violation sets kStatusBounds,
// records (site tag, offending value) of the first one in counters[kCtrBoundsTag .. kCtrBoundsHi] and the access is skipped instead of made.
// It is the address sanitizer this pool does not offer for the GPU (tests/test_gpu_parity.py runs the suite's scenes
// through it once).  In the product build TOPO_CHK is `true` and costs nothing.
#ifdef TOPO_BOUNDS_CHECK
__device__ __noinline__ void bounds_violation(uint32_t* counters, uint32_t tag, uint64_t value) {
    if ((atomicOr(&counters[kCtrStatus], kStatusBounds) & kStatusBounds) == 0) {
        counters[kCtrBoundsTag] = tag;
        counters[kCtrBoundsLo] = (uint32_t)value;
        counters[kCtrBoundsHi] = (uint32_t)(value >> 32);
    }
}
#define TOPO_CHK(counters, ok, tag, value) ((ok) ? true : (bounds_violation((counters), (tag), (uint64_t)(value)), false))
#else
#define TOPO_CHK(counters, ok, tag, value) true
#endif

__device__ __forceinline__ Vis view_vis(const FrameParams& P, uint32_t view) {
#ifdef TOPO_BOUNDS_CHECK
    (void)TOPO_CHK(P.counters, view < P.n_views, 1u, view);
    return Vis{P.vis + (size_t)view * P.W * P.H, P.vis, P.dirty, P.counters, (size_t)P.W * P.H};
#else
    return Vis{P.vis + (size_t)view * P.W * P.H, P.vis, P.dirty};
#endif
}
// the atomic alone, for callers that mark the segments themselves (k_raster_big: once per item and pixel row)
__device__ __forceinline__ void vis_min_unmarked(const Vis& v, size_t pix, uint64_t key) {
#ifdef TOPO_BOUNDS_CHECK
    if (!TOPO_CHK(v.counters, pix < v.view_keys, 2u, pix)) return;
#endif
    atomicMin(reinterpret_cast<unsigned long long*>(v.p + pix), (unsigned long long)key);
}
__device__ __forceinline__ void vis_min(const Vis& v, size_t pix, uint64_t key) {
#ifdef TOPO_BOUNDS_CHECK
    if (!TOPO_CHK(v.counters, pix < v.view_keys, 2u, pix)) return;
#endif
    uint64_t* q = v.p + pix;
    atomicMin(reinterpret_cast<unsigned long long*>(q), (unsigned long long)key);
    v.dirty[(size_t)(q - v.base) >> 6] = 1;
}

// ---- wave helpers --------------------------------------------------------------------------------------

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));         // a pair of floats at any 4-byte boundary
typedef uint32_t u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));

// A wave's LDS tables are written and read by that wave alone, and a wave's LDS operations complete in order; what the
// hardware does not promise is that the COMPILER keeps a lane's read behind another lane's write to a different address.
// This fence (no instruction: it only orders the compiler's memory operations within the wave) stands between every write
// phase and the read phase that follows it.
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// The first active lane's value, wave-uniform: for a value that IS the same in every lane but that the compiler cannot know to be,
// this says so -- it moves to a scalar register, and so does everything computed from it.
__device__ __forceinline__ int32_t wave_first(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t wave_first(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)v); }
__device__ __forceinline__ float wave_first(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
// lane `src_lane`'s value (a wave-uniform lane number), wave-uniform
__device__ __forceinline__ float wave_lane(float v, int src_lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src_lane)); }
__device__ __forceinline__ double shfl_f64(double v, int src) {
    return __hiloint2double(__shfl(__double2hiint(v), src), __shfl(__double2loint(v), src));
}
__device__ __forceinline__ double shfl_xor_f64(double v, int mask) {
    return __hiloint2double(__shfl_xor(__double2hiint(v), mask), __shfl_xor(__double2loint(v), mask));
}
// lane `src`'s value for a wave-uniform src: scalar registers
__device__ __forceinline__ double lane_f64(double v, int src) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}
__device__ __forceinline__ uint32_t pop_bit(uint64_t& m) {      // wave-uniform mask: scalar instructions
    const uint32_t j = (uint32_t)__builtin_ctzll(m);
    m &= m - 1ull;
    return j;
}
__device__ __forceinline__ float wave_from_left(float v, float first) {      // lane i: lane i - 1's v; lane 0: `first`
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(first), __float_as_int(v), 0x138 /* wave_shr:1 */, 0xF, 0xF, false));
}
__device__ __forceinline__ float wave_from_right(float v, float last) {      // lane i: lane i + 1's v; lane 63: `last`
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(last), __float_as_int(v), 0x130 /* wave_shl:1 */, 0xF, 0xF, false));
}

// `p`, read through the constant address space: for wave-uniform data that an EARLIER launch wrote (or the launch's own argument
// segment).  Such loads go over the scalar data path (s_load, scalar cache) and are waited for on lgkmcnt; as vector loads they
// are waited for with s_waitcnt vmcnt(0), which also waits for every vector load, store and atomic the wave still has in flight.
template <typename T>
using const_space_ptr = const __attribute__((address_space(4))) T*;
template <typename T>
__device__ __forceinline__ const_space_ptr<T> const_space(const T* p) {
    return (const_space_ptr<T>)(const void*)p;
}
// the kernel's own argument segment, `offset` bytes in, as T
template <typename T>
__device__ __forceinline__ const_space_ptr<T> kernarg(size_t offset = 0) {
    return (const_space_ptr<T>)((const_space_ptr<uint8_t>)__builtin_amdgcn_kernarg_segment_ptr() + offset);
}

}  // namespace
}  // namespace topo
