// fa_paged_fp8_launch.h -- internal seam between the FP8 paged C-ABI dispatcher (fa_paged_fp8_gfx950.hip)
// and the FP8 paged decode instantiations (fa_paged_fp8_inst.hip x 16), beside fa_paged_launch.h: the
// 16-bit dispatchers and their instantiations never see these declarations.
#pragma once

#include "fa_paged_launch.h"

namespace fa {

// fa_debug_last_path values of the FP8 paged decode (after fa_launch.h's Path)
constexpr int kPathDecodePagedFp8 = 11, kPathDecodePagedFp8Split = 12;

// PagedDecArgs plus the descales (fa_decode_paged_fp8.hpp). In the fa_fwd_params that go with it the k / v
// pointers and strides describe 1-byte e4m3 elements; q / o are the 16-bit DT.
struct PagedFp8DecArgs : PagedDecArgs {
    const float *k_descale, *v_descale;  // [B, Hkv] fp32, device; nullptr: 1.0
    int64_t descale_batch_stride, descale_head_stride;
};

// The split plan (shared by the FP8 dispatcher and the sliding-window dispatcher): decode_plan's rule (every wave at least kDecMinTilesPerWave tiles, at most kDecMaxSplit
// splits) aiming at kFp8DecTargetWgs workgroups instead of kDecTargetWgs. A workgroup streams half the bytes
// per key here, and the measured optimum moves from "fewer, longer splits" to one workgroup per CU: B1 Hkv8
// 131072 keys, same process, 0.0814 / 0.0635 / 0.0555 / 0.0486 / 0.0484 ms at 96 / 128 / 160 / 192 / 256
// workgroups (profiles/fp8_decode_target_ab.json). A dec_target knob that was moved off its default wins.
constexpr int64_t kFp8DecTargetWgs = 256;

inline DecArgs fp8_decode_plan(const fa_fwd_params &p, int max_split) {
    DecArgs a = decode_plan(p, max_split);
    if (knobs().dec_target != kDecTargetWgs) return a;
    const int64_t units = decode_units(p, a);
    const int n_tiles = (int)((p.seqlen_kv + kDecKeys - 1) / kDecKeys);
    int64_t ns = (kFp8DecTargetWgs + units - 1) / units;
    const int64_t by_len = n_tiles / (kDecWaves * kDecMinTilesPerWave);
    ns = ns < by_len ? ns : by_len;
    ns = ns < max_split ? ns : max_split;
    ns = ns < 1 ? 1 : ns;
    a.tps = (int)((n_tiles + ns - 1) / ns);
    a.n_split = (n_tiles + a.tps - 1) / a.tps;
    return a;
}

template <class DT, bool C, int kD, bool kExact>
int launch_decode_paged_fp8(const fa_fwd_params &p, PagedFp8DecArgs a, void *ws, hipStream_t stream);

#define FA_DECLARE_EXTERN_PAGED_FP8(DT, C, D, E)                                                        \
    extern template int launch_decode_paged_fp8<DT, C, D, E>(const fa_fwd_params &, PagedFp8DecArgs, void *, \
                                                             hipStream_t);
FA_FOR_EACH_INSTANCE(FA_DECLARE_EXTERN_PAGED_FP8)
#undef FA_DECLARE_EXTERN_PAGED_FP8

}  // namespace fa
