// mpc_wave_layout.hpp -- the wave kernel's stage-record slot tables, scalar slots and wavefront reductions (device); the layouts themselves are mpc_layout.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <utility>

#include "mpc_core.hpp"
#include "mpc_layout.hpp"

namespace mpc {

enum { SC_D = 0, SC_DT = 1, SC_DD = 2, SC_PDL = 3, SC_PDU = 4, SC_TS = 5, SC_TY = 6, SC_TG = 7, SC_TA = 8 /* 8..10 */ };

// A slot (StageAdd) of the entry (r, c) of the symmetric 8x8 stage cost block [x(3) u_prev(2) dt u(2)] and of its gradient
// column c = 8; -1 where the block is structurally zero.  Packed per row as 12 x 5 bits (slot + 1) so that a lane looks its
// column up with one 64-bit shift instead of a cascade of divergent branches.
constexpr int stage_add_slot(int r, int c, bool ext) {
    if (c == 8) return A08 + r;
    if (c > 8) return -1;
    const int a = r < c ? r : c, b = r < c ? c : r;
    if (a == 0) return b == 0 ? A00 : (b == 1 ? A01 : (b == 2 && ext ? A02 : (b == 5 && ext ? A05 : -1)));
    if (a == 1) return b == 1 ? A11 : (b == 2 && ext ? A12 : (b == 5 && ext ? A15 : -1));
    if (a == 2) return b == 2 ? A22 : (b == 5 ? A25 : (b == 6 ? A26 : (b == 7 ? A27 : -1)));
    if (a == 3) return b == 3 ? A33 : (b == 5 ? A35 : (b == 6 ? A36 : -1));
    if (a == 4) return b == 4 ? A44 : (b == 5 ? A45 : (b == 7 ? A47 : -1));
    if (a == 5) return b == 5 ? A55 : (b == 6 ? A56 : (b == 7 ? A57 : -1));
    if (a == 6) return b == 6 ? A66 : (b == 7 ? A67 : -1);
    return b == 7 ? A77 : -1;
}
constexpr unsigned long long stage_add_row(int r, bool ext) {
    unsigned long long v = 0;
    for (int c = 0; c < 12; ++c) v |= (unsigned long long)(stage_add_slot(r, c, ext) + 1) << (5 * c);
    return v;
}


// ---- wavefront reductions on the DPP path, no LDS traffic: row rotations inside each 16-lane row (row_ror 8, 4, 2, 1: every lane of a row then holds the row's
//      reduction), row_bcast:15 into rows 1 and 3, row_bcast:31 into row 3, and ONE v_readlane pair of lane 63: 20 VALU instructions per fp64 sum, wave-uniform
//      result -- 27 issued: every step opens with `s_nop 1` (the two wait states between a VALU write and a DPP read of it) and an `s_nop 0` stands in front of the
//      readlanes; a fp64 min / max is a compare and two selects per step with two more wait states between them, 44 in all.  A pass with several reductions uses
//      wave_reduce_n() below where the kernel allows it.  The moves name no "old" value (an undefined register: every lane that is read later is written), which spares
//      a copy per move; row 3 ends up with (r3 + r2) + (r1 + r0) -- the association the earlier readlane version had.
__device__ __forceinline__ int undef_vgpr() { int x; asm volatile("" : "=v"(x)); return x; }
template <int CTRL, int ROWS = 0xf> __device__ __forceinline__ double dpp_mov(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(undef_vgpr(), lo, CTRL, ROWS, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(undef_vgpr(), hi, CTRL, ROWS, 0xf, false);
    return __hiloint2double(hi, lo);
}
template <int CTRL, int ROWS = 0xf> __device__ __forceinline__ float dpp_mov(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(undef_vgpr(), __float_as_int(v), CTRL, ROWS, 0xf, false));
}
__device__ __forceinline__ double rd_lane(double v, int src) {
    int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float rd_lane(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }
// the value of lane `src` (per-lane index) in every lane: ds_bpermute on the 32-bit halves
__device__ __forceinline__ double lane_gather(double v, int src) {
    const int lo = __builtin_amdgcn_ds_bpermute(4 * src, __double2loint(v)), hi = __builtin_amdgcn_ds_bpermute(4 * src, __double2hiint(v));
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float lane_gather(float v, int src) { return __int_as_float(__builtin_amdgcn_ds_bpermute(4 * src, __float_as_int(v))); }

struct OpSum { template <typename T> __device__ __forceinline__ static T f(T a, T b) { return a + b; } };
struct OpMin { template <typename T> __device__ __forceinline__ static T f(T a, T b) { return b < a ? b : a; } };
struct OpMax { template <typename T> __device__ __forceinline__ static T f(T a, T b) { return b > a ? b : a; } };

template <typename Op, typename T> __device__ __forceinline__ T wave_reduce(T v) {
    // row_ror:8,4,2,1 (dpp_ctrl 0x120 + n): afterwards every lane of a row holds the row's reduction
    v = Op::f(v, dpp_mov<0x128>(v));
    v = Op::f(v, dpp_mov<0x124>(v));
    v = Op::f(v, dpp_mov<0x122>(v));
    v = Op::f(v, dpp_mov<0x121>(v));
    v = Op::f(v, dpp_mov<0x142, 0xa>(v));      // row_bcast:15 -> rows 1, 3 (the other rows' lanes are never read again)
    v = Op::f(v, dpp_mov<0x143, 0x8>(v));      // row_bcast:31 -> row 3
    return rd_lane(v, 63);
}
// The reductions of one pass carried through the six steps TOGETHER: at every step the DPP moves of all K values, then the K operations; the K readlane pairs at the
// end.  Each value sees wave_reduce()'s sequence and operand order, so its result is wave_reduce<Op>()'s bit for bit.  What changes is what stands between a value's
// operation and the DPP move that reads it next (two wait states): the other values' instructions instead of the `s_nop 1` a lone chain pays at every step -- and the
// undefined "old" value comes from the mov_dpp builtin, not from an empty asm: the compiler pads a DPP move behind an asm that defines one of its registers as it pads
// one behind a VALU write, so wave_reduce() pays its `s_nop 1` even where the value itself is old.  The compiler still owns every hazard here; the scheduling barrier
// behind a step only keeps it in front of the next one (it emits nothing).  Inside a step the scheduler is free: it fills the two wait states between a compare and
// the selects that read its mask with the other values' moves.
template <int CTRL, int ROWS> __device__ __forceinline__ double dpp_mov_n(double v) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, ROWS, 0xf, false), hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, ROWS, 0xf, false);
    return __hiloint2double(hi, lo);
}
template <int CTRL, int ROWS> __device__ __forceinline__ float dpp_mov_n(float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, ROWS, 0xf, false)); }
template <int CTRL, int ROWS, typename... Ops, typename T, size_t... I> __device__ __forceinline__ void wave_reduce_step_n(T (&v)[sizeof...(Ops)], std::index_sequence<I...>) {
    const T t[sizeof...(Ops)] = {dpp_mov_n<CTRL, ROWS>(v[I])...};
    ((v[I] = Ops::f(v[I], t[I])), ...);
    __builtin_amdgcn_sched_barrier(0);
}
template <typename... Ops, typename T> __device__ __forceinline__ void wave_reduce_n(T (&v)[sizeof...(Ops)]) {
    constexpr auto is = std::make_index_sequence<sizeof...(Ops)>{};
    __builtin_amdgcn_sched_barrier(0);
    wave_reduce_step_n<0x128, 0xf, Ops...>(v, is);
    wave_reduce_step_n<0x124, 0xf, Ops...>(v, is);
    wave_reduce_step_n<0x122, 0xf, Ops...>(v, is);
    wave_reduce_step_n<0x121, 0xf, Ops...>(v, is);
    wave_reduce_step_n<0x142, 0xa, Ops...>(v, is);      // row_bcast:15 -> rows 1, 3
    wave_reduce_step_n<0x143, 0x8, Ops...>(v, is);      // row_bcast:31 -> row 3
#pragma unroll
    for (int i = 0; i < (int)sizeof...(Ops); ++i) v[i] = rd_lane(v[i], 63);
}
template <typename T> __device__ __forceinline__ T wave_sum(T v) { return wave_reduce<OpSum>(v); }
template <typename T> __device__ __forceinline__ T wave_min(T v) { return wave_reduce<OpMin>(v); }
template <typename T> __device__ __forceinline__ T wave_max(T v) { return wave_reduce<OpMax>(v); }

__device__ __forceinline__ double lane_bcast(double v, int src) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, src);
    hi = __builtin_amdgcn_readlane(hi, src);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float lane_bcast(float v, int src) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

}  // namespace mpc
