// fp32 -> the two 16-bit operand planes of a VD_PREC_* format: hi = rn16(v), lo = rn16(v - hi), in bf16 for the bf16 formats and
// in fp16 for the others.  One definition for every kernel that writes 16-bit operands (aux_kernels.hip, still_rows.hip), so
// that two writers of one layout cannot drift apart.  Needs VD_PREC_* (include/vd_hip.h) in front of it.
#ifndef VD_SPLIT16_H
#define VD_SPLIT16_H

#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ void split16p(int prec, float v, uint16_t& hi, uint16_t& lo) {
    if (prec == VD_PREC_BF16 || prec == VD_PREC_BF16X3) {
        __bf16 h = (__bf16)v;
        __bf16 l = (__bf16)(v - (float)h);
        hi = __builtin_bit_cast(uint16_t, h);
        lo = __builtin_bit_cast(uint16_t, l);
    } else {
        _Float16 h = (_Float16)v;
        _Float16 l = (_Float16)(v - (float)h);
        hi = __builtin_bit_cast(uint16_t, h);
        lo = __builtin_bit_cast(uint16_t, l);
    }
}

#endif /* VD_SPLIT16_H */
