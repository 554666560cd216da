// The argument checks every int8 GEMM entry point (qlinear*.hip) makes, stated once: host code only.
// An entry point first checks what is its own -- a row range, a narrower w_format or G with its "(... runs on ...)"
// hint, a k-unit -- in its own words, then returns the status of one of the two functions below; what it has
// narrowed already passes the wider check here.  `name` is the entry point's, the prefix of every message.
#pragma once
#include "common.h"

// the part of both lists behind "bad arguments"; aligned16: the form fetches Xq and Wq 16 bytes at a time
static inline int qt_i8_check_shared(const char* name, bool args_ok, const void* Xq, int K, const void* Wq, int w_format,
                                     const void* zp_x, int G, const void* wsum, int out_dtype, bool aligned16) {
    QT_CHECK_ARG(args_ok, "%s: bad arguments", name);
    QT_CHECK_ARG(K <= 32768, "%s: K %d > 32768 (the int32 accumulator bound)", name, K);
    QT_CHECK_ARG(w_format == QT_W_INT8 || w_format == QT_W_INT4_PACKED, "%s: w_format %d unsupported", name, w_format);
    QT_CHECK_ARG(qt_dtype_is16(out_dtype), "%s: out_dtype %d must be bf16 or fp16", name, out_dtype);
    QT_CHECK_ARG(G == 1 || G == (K + 127) / 128, "%s: G %d must be 1 or ceil(K / 128) = %d", name, G, (K + 127) / 128);
    QT_CHECK_ARG(!zp_x || wsum, "%s: zp_x needs wsum", name);
    QT_CHECK_ARG(!aligned16 || ((uintptr_t)Xq & 15) == 0, "%s: Xq is not 16-byte aligned", name);
    QT_CHECK_ARG(!aligned16 || ((uintptr_t)Wq & 15) == 0, "%s: Wq is not 16-byte aligned", name);
    return QT_OK;
}

// qt_gemm_i8's arguments (M an int in qt_gemm_i8_skinny)
static inline int qt_i8_check_dense(const char* name, const void* Xq, int64_t M, int K, const void* Wq, int w_format,
                                    int N, const void* s_x, const void* zp_x, const void* s_w, int G, const void* wsum,
                                    const void* Y, int out_dtype, int64_t ldy, bool aligned16 = false) {
    return qt_i8_check_shared(name, Xq && Wq && s_x && s_w && Y && M > 0 && N > 0 && K > 0 && ldy >= N, Xq, K, Wq,
                              w_format, zp_x, G, wsum, out_dtype, aligned16);
}

// qt_gemm_i8_grouped's arguments
static inline int qt_i8_check_grouped(const char* name, const void* Xq, int K, int64_t R, const void* offsets, int E,
                                      const void* Wq, int w_format, int N, const void* s_x, const void* zp_x,
                                      const void* s_w, int G, const void* wsum, const void* Y, int out_dtype,
                                      int64_t ldy, bool aligned16 = false) {
    const bool args_ok = Xq && Wq && offsets && s_x && s_w && Y && R > 0 && E > 0 && N > 0 && K > 0 && ldy >= N;
    if (int st = qt_i8_check_shared(name, args_ok, Xq, K, Wq, w_format, zp_x, G, wsum, out_dtype, aligned16)) return st;
    QT_CHECK_ARG(R <= 0x7fffffffLL && E <= 4096, "%s: R %lld or E %d too large", name, (long long)R, E);
    return QT_OK;
}
