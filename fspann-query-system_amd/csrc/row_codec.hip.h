// row_codec.hip.h — what the kernels know about each row element type, in ONE place: RowCodec<T>, one specialisation per row of
// FSPANN_DTYPE_TABLE (dtypes.h).  How a row's bits become a value, and whether that value is finite, is a data format; every
// kernel that reads rows (the Refine scans, the typed ground truth, its validator and the evaluation sweep, Setup's widening, the
// touched-record set) takes it from here.  Included from fspann_common.h behind dtypes.h.
//
// A codec holds:
//   slot               the native 16-byte vector the Refine scan keeps a piece of a row in (a plain SSA value: a HIP float4 staging
//                      array ends up in scratch)
//   N                  elements per 16-byte slot, 16 / sizeof(T); a plain constant, the host computes with it too
//   always_finite      DtypeOf<T>::finite: no element of the type can be NaN or infinite
//   wide(slot, e)      element e of a slot widened EXACTLY to fp64 (e is a constant after unrolling)
//   piece_f32(p, e)    element e of a 16-byte piece held as four dwords (fsp_u32x4: what the ground-truth kernels load), widened
//                      EXACTLY to fp32; every type but double has it, every value of those types is a float, so nothing rounds
//   quad_f32(in)         four consecutive elements (4-byte aligned for the byte types, 8-byte for the 16-bit ones) widened exactly to
//                      fp32: Setup's input of a row-only type
//   finite(x)          one raw element is finite
//   fits(x)            the inverse direction (narrow.hip.h; every type but double): the fp32 or fp64 value x IS a value of T — nothing
//                      is ever rounded, shifted or scaled.  The rule per type is engine._typed_rows' on the host; an fp64 x fits iff it
//                      is a float and that float fits (every value of a narrower type is a float)
//   narrow(x)          the element of a value that fits (a NaN becomes some NaN of T; of a value that does not fit: unspecified)
//   slot_test          the granularity in which the Refine scan, which walks a slot two elements at a time, asks it for finiteness:
//                      SlotTest::element  slot_finite(slot, e), one raw element (the scan: ok && slot_finite(e) && slot_finite(e + 1));
//                      SlotTest::pair     pair_finite(slot, e), elements e and e + 1 (the scan: ok && pair_finite(e));
//                      SlotTest::none     nothing to ask.
//                      The scan spells the `&&` chain itself, from these pieces: its association is part of the scans' generated
//                      code ((ok && a) && b and ok && (a && b) schedule differently), and so is whether `ok` passes through a call.
// Kernels keep fp16 and fp32 denormals (float_denorm_mode_16_64 = 3, float_denorm_mode_32 = 3), so a subnormal half or bfloat16
// arrives as its value.
#pragma once

namespace fspann {

typedef float fsp_f32x4 __attribute__((ext_vector_type(4)));
typedef double fsp_f64x2 __attribute__((ext_vector_type(2)));
typedef uint32_t fsp_u32x4 __attribute__((ext_vector_type(4)));
typedef uint64_t fsp_u64x2 __attribute__((ext_vector_type(2)));

enum class SlotTest { none, element, pair };
template <typename T> struct RowCodec;
template <typename T, typename Slot> struct RowCodecOf {
    using slot = Slot;
    static constexpr int N = 16 / static_cast<int>(sizeof(T));
    static constexpr bool always_finite = DtypeOf<T>::finite;
};
// The types a slot holds as themselves (float, double, _Float16): an element is tested with v_cmp_class on the raw element.
template <typename T, typename Slot> struct NativeRowCodec : RowCodecOf<T, Slot> {
    static __device__ __forceinline__ bool finite(T x) { return __builtin_isfinite(x); }
    static constexpr SlotTest slot_test = SlotTest::element;
    static __device__ __forceinline__ bool slot_finite(Slot v, int e) { return __builtin_isfinite(v[e]); }
};
// The byte types (uint8_t, int8_t): a 16-byte slot is 16 elements, byte e of the slot = bits [8 (e % 4), 8 (e % 4) + 8) of dword
// e / 4.  A byte is always finite, so no row element is ever tested.
template <typename T, typename Slot> struct ByteRowCodec : RowCodecOf<T, Slot> {
    static __device__ __forceinline__ bool finite(T) { return true; }
    static constexpr SlotTest slot_test = SlotTest::none;
};

// FSPANN_F32: the element itself; float -> double is exact.
template <> struct RowCodec<float> : NativeRowCodec<float, fsp_f32x4> {
    static __device__ __forceinline__ double wide(slot v, int e) { return static_cast<double>(v[e]); }
    static __device__ __forceinline__ float piece_f32(fsp_u32x4 p, int e) { return __uint_as_float(p[e]); }
    // an fp64 value is a float iff it survives the round trip by value (+-inf does; a NaN stays a NaN)
    static __device__ __forceinline__ bool fits(double x) { return static_cast<double>(static_cast<float>(x)) == x || x != x; }
    static __device__ __forceinline__ float narrow(double x) { return static_cast<float>(x); }
};

// FSPANN_F64: the element itself.  No kernel reads fp64 rows as fp32 pieces, and Setup takes them as they are.
template <> struct RowCodec<double> : NativeRowCodec<double, fsp_f64x2> {
    static __device__ __forceinline__ double wide(slot v, int e) { return v[e]; }
};

// FSPANN_U8: a row element is the integer 0..255; the slot is held as four unsigned dwords.
template <> struct RowCodec<uint8_t> : ByteRowCodec<uint8_t, fsp_u32x4> {
    // A bit-field extract and v_cvt_f64_u32.  Measured against v_cvt_f32_ubyte0..3 + v_cvt_f64_f32, against building 2^52 + byte in
    // the mantissa and subtracting 2^52 (no conversion at all), and against keeping the query's tile as fp64 in LDS instead of
    // converting it per element: within 5 % of each other — every vector instruction of the scan's loop issues at
    // the same rate, so the plain expression stays.
    static __device__ __forceinline__ double wide(slot v, int e) { return static_cast<double>((v[e >> 2] >> (8 * (e & 3))) & 0xFFu); }
    // v_cvt_f32_ubyte0..3
    static __device__ __forceinline__ float piece_f32(fsp_u32x4 p, int e) { return static_cast<float>((p[e >> 2] >> (8 * (e & 3))) & 0xffu); }
    // a bit-field extract and an integer conversion per element
    static __device__ __forceinline__ float4 quad_f32(const uint8_t* __restrict__ in) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(in);
        return make_float4(static_cast<float>(w & 0xFFu), static_cast<float>((w >> 8) & 0xFFu), static_cast<float>((w >> 16) & 0xFFu), static_cast<float>(w >> 24));
    }
    // In 0..255 (a NaN is not; -0.0 is, and narrows to 0: no result depends on that sign), and an integer: it
    // survives v_cvt_i32_f32 and the way back.
    static __device__ __forceinline__ bool fits(float x) { return x >= 0.0f && x <= 255.0f && static_cast<float>(static_cast<int32_t>(x)) == x; }
    static __device__ __forceinline__ uint8_t narrow(float x) { return static_cast<uint8_t>(static_cast<int32_t>(x)); }
    static __device__ __forceinline__ bool fits(double x) { return RowCodec<float>::fits(x) && fits(static_cast<float>(x)); }
    static __device__ __forceinline__ uint8_t narrow(double x) { return narrow(static_cast<float>(x)); }
    // the byte ground truth's matrix cores take SIGNED bytes: x ^ 0x80 = x - 128 (groundtruth_u8.hip.h)
    static constexpr unsigned kToSigned = 0x80u;
};

// FSPANN_I8: a row element is the two's-complement integer -128..127.  The slot is held as two qwords, a native vector like the
// others: sixteen separate bytes would be the natural spelling, but a conditional load of such a vector is legalised byte by byte
// and ends in scratch.
template <> struct RowCodec<int8_t> : ByteRowCodec<int8_t, fsp_u64x2> {
    // The byte's sign is extended by a left shift to the top of its dword and an arithmetic shift back (one v_bfe_i32; for the top
    // byte the arithmetic shift alone) ...
    static __device__ __forceinline__ int32_t sext(fsp_u32x4 p, int e) { return static_cast<int32_t>(p[e >> 2] << (24 - 8 * (e & 3))) >> 24; }
    // ... then v_cvt_f64_i32 — the instruction count of the unsigned byte
    static __device__ __forceinline__ double wide(slot v, int e) { return static_cast<double>(sext(__builtin_bit_cast(fsp_u32x4, v), e)); }
    // v_cvt_f32_i32 of the sign-extended byte (SDWA sext)
    static __device__ __forceinline__ float piece_f32(fsp_u32x4 p, int e) { return static_cast<float>(sext(p, e)); }
    static __device__ __forceinline__ float4 quad_f32(const int8_t* __restrict__ in) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(in);
        return make_float4(static_cast<float>(static_cast<int32_t>(w << 24) >> 24), static_cast<float>(static_cast<int32_t>(w << 16) >> 24),
                           static_cast<float>(static_cast<int32_t>(w << 8) >> 24), static_cast<float>(static_cast<int32_t>(w) >> 24));
    }
    static constexpr unsigned kToSigned = 0u;      // already signed; ^ 0 compiles to nothing
    // an integer in -128..127 (the test of FSPANN_U8 over another range)
    static __device__ __forceinline__ bool fits(float x) { return x >= -128.0f && x <= 127.0f && static_cast<float>(static_cast<int32_t>(x)) == x; }
    static __device__ __forceinline__ int8_t narrow(float x) { return static_cast<int8_t>(static_cast<int32_t>(x)); }
    static __device__ __forceinline__ bool fits(double x) { return RowCodec<float>::fits(x) && fits(static_cast<float>(x)); }
    static __device__ __forceinline__ int8_t narrow(double x) { return narrow(static_cast<float>(x)); }
};

// FSPANN_F16: a 16-byte slot is 8 IEEE binary16 elements (four dwords, two halves each, low element in the low 16 bits).  An
// element is the half widened exactly (half -> float -> double: every finite half, subnormals included, is a double), and unlike a
// byte it can be +-inf or NaN.
typedef _Float16 fsp_f16x8 __attribute__((ext_vector_type(8)));
template <> struct RowCodec<_Float16> : NativeRowCodec<_Float16, fsp_f16x8> {
    // v_cvt_f32_f16 (the high half of a dword through SDWA src0_sel:WORD_1, no shift), then v_cvt_f64_f32
    static __device__ __forceinline__ double wide(slot v, int e) { return static_cast<double>(static_cast<float>(v[e])); }
    // the same v_cvt_f32_f16 (WORD_1 for the high half)
    static __device__ __forceinline__ float piece_f32(fsp_u32x4 p, int e) {
        return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>((e & 1) ? (p[e >> 1] >> 16) : (p[e >> 1] & 0xffffu))));
    }
    // v_cvt_f32_f16, subnormals, infinities and NaN included
    static __device__ __forceinline__ float4 quad_f32(const _Float16* __restrict__ in) {
        typedef _Float16 h4 __attribute__((ext_vector_type(4)));
        const h4 w = *reinterpret_cast<const h4*>(in);
        return make_float4(static_cast<float>(w[0]), static_cast<float>(w[1]), static_cast<float>(w[2]), static_cast<float>(w[3]));
    }
    // the round trip by value (v_cvt_f16_f32 and back): whichever way the conversion rounds, it gives x back iff x is a half;
    // 65520 becomes +inf and does not fit, +-inf and NaN do
    static __device__ __forceinline__ bool fits(float x) { return static_cast<float>(static_cast<_Float16>(x)) == x || x != x; }
    static __device__ __forceinline__ _Float16 narrow(float x) { return static_cast<_Float16>(x); }
    static __device__ __forceinline__ bool fits(double x) { return RowCodec<float>::fits(x) && fits(static_cast<float>(x)); }
    static __device__ __forceinline__ _Float16 narrow(double x) { return narrow(static_cast<float>(x)); }
};

// FSPANN_BF16: the 2-byte geometry of FSPANN_F16.  An element is the fp32 whose bit pattern is the 16 bits shifted up, and can be
// +-inf or NaN.  The slot is held as four dwords, the slot of FSPANN_U8: a native vector like the others (a struct could not be a
// nontemporal load's result), and at the same time a 16-byte piece.  The low element of a dword is dword << 16, the high one dword & 0xffff0000, each taken as the bits of a float —
// one integer VALU op and no conversion that could round; nothing depends on the fp16 denormal mode, but a bf16 subnormal is an
// fp32 subnormal and must survive v_cvt_f64_f32.
template <> struct RowCodec<fsp_bf16> : RowCodecOf<fsp_bf16, fsp_u32x4> {
    // the 16 bits moved to the top of a dword
    static __device__ __forceinline__ float piece_f32(fsp_u32x4 p, int e) { return __uint_as_float((e & 1) ? (p[e >> 1] & 0xffff0000u) : (p[e >> 1] << 16)); }
    static __device__ __forceinline__ double wide(slot v, int e) { return static_cast<double>(piece_f32(v, e)); }
    static __device__ __forceinline__ float4 quad_f32(const fsp_bf16* __restrict__ in) {
        const uint2 w = *reinterpret_cast<const uint2*>(in);
        return make_float4(__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u), __uint_as_float(w.y << 16), __uint_as_float(w.y & 0xffff0000u));
    }
    // an element is +-inf or NaN iff its exponent field is all ones
    static __device__ __forceinline__ bool finite(fsp_bf16 x) { return (x.b & 0x7f80u) != 0x7f80u; }
    // In the scan that exponent field is the widened float's: one v_cmp_class_f32 on the float the widening has made anyway, instead
    // of a mask and a compare on the raw dword.
    static __device__ __forceinline__ bool pair_finite(slot v, int e) { return __builtin_isfinite(piece_f32(v, e)) && __builtin_isfinite(piece_f32(v, e + 1)); }
    static constexpr SlotTest slot_test = SlotTest::pair;
    // the low 16 bits of the fp32 pattern are zero; a NaN fits whatever its payload
    static __device__ __forceinline__ bool fits(float x) { return (__float_as_uint(x) & 0xffffu) == 0 || x != x; }
    // the upper 16 bits; a NaN whose payload sat in the low bits only stays a NaN (the wrapper's rule)
    static __device__ __forceinline__ fsp_bf16 narrow(float x) {
        uint32_t hi = __float_as_uint(x) >> 16;
        if (x != x && (hi & 0x7fu) == 0) hi |= 0x40u;
        return fsp_bf16{static_cast<uint16_t>(hi)};
    }
    static __device__ __forceinline__ bool fits(double x) { return RowCodec<float>::fits(x) && fits(static_cast<float>(x)); }
    static __device__ __forceinline__ fsp_bf16 narrow(double x) { return narrow(static_cast<float>(x)); }
};

// FSPANN_F8E4M3: the byte geometry of FSPANN_U8.  An element is an OCP e4m3fn value and, unlike a byte, can be NaN (0x7F / 0xFF;
// the format has no infinity, |x| <= 448).  The slot is held as two qwords, for the reason given at FSPANN_I8 (sixteen
// separate bytes cost 384-396 bytes of scratch).  The widening is the hardware's OCP e4m3fn conversion of dword e / 4 — every e4m3
// value, subnormals included, is a normal fp32, so nothing depends on a denormal mode.
// Which hardware conversion widens a slot (both exact; a switch so that the two can be A/B-ed): 0 = v_cvt_pk_f32_fp8,
// one instruction per two elements (the word of the dword through SDWA src0_sel:WORD_1; the two elements of a pair (e, e + 1) come
// out of one instruction); 1 = v_cvt_f32_fp8, one per element (the byte through SDWA src0_sel:BYTE_n).
#ifndef FSPANN_F8_WIDEN
#define FSPANN_F8_WIDEN 0
#endif
template <> struct RowCodec<fsp_f8e4m3> : RowCodecOf<fsp_f8e4m3, fsp_u64x2> {
    // one v_cvt_pk_f32_fp8 per pair
    static __device__ __forceinline__ float piece_f32(fsp_u32x4 p, int e) {
        const int w = static_cast<int>(p[e >> 2]);
        return (e & 2) ? __builtin_amdgcn_cvt_pk_f32_fp8(w, true)[e & 1] : __builtin_amdgcn_cvt_pk_f32_fp8(w, false)[e & 1];
    }
    static __device__ __forceinline__ float slot_f32(slot v, int e) {
#if FSPANN_F8_WIDEN == 0
        return piece_f32(__builtin_bit_cast(fsp_u32x4, v), e);
#else
        const int w = static_cast<int>(__builtin_bit_cast(fsp_u32x4, v)[e >> 2]);
        switch (e & 3) {
        case 0: return __builtin_amdgcn_cvt_f32_fp8(w, 0);
        case 1: return __builtin_amdgcn_cvt_f32_fp8(w, 1);
        case 2: return __builtin_amdgcn_cvt_f32_fp8(w, 2);
        default: return __builtin_amdgcn_cvt_f32_fp8(w, 3);
        }
#endif
    }
    static __device__ __forceinline__ double wide(slot v, int e) { return static_cast<double>(slot_f32(v, e)); }
    // two v_cvt_pk_f32_fp8 per dword
    static __device__ __forceinline__ float4 quad_f32(const fsp_f8e4m3* __restrict__ in) {
        typedef float f2 __attribute__((ext_vector_type(2)));
        const int w = *reinterpret_cast<const int*>(in);
        const f2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
        return make_float4(lo[0], lo[1], hi[0], hi[1]);
    }
    // an element is NaN iff all seven bits under the sign are set
    static __device__ __forceinline__ bool finite(fsp_f8e4m3 x) { return (x.b & 0x7fu) != 0x7fu; }
    // In the scan the four bytes of a dword are tested at once, with the dword's first pair: under the mask 0x7f7f7f7f adding 1 to
    // every byte carries into its bit 7 iff its seven bits were all ones, and never into the next byte — three integer operations
    // per four elements, nothing for the second pair.
    static __device__ __forceinline__ bool pair_finite(slot v, int e) {
        if (e & 2) return true;
        const uint32_t w = __builtin_bit_cast(fsp_u32x4, v)[e >> 2];
        return (((w & 0x7f7f7f7fu) + 0x01010101u) & 0x80808080u) == 0;
    }
    static constexpr SlotTest slot_test = SlotTest::pair;
    // u = |x| * 2^9 as an integer (the scaling is exact; |x| <= 448 keeps it below 2^18): x is an e4m3 value iff t is that integer and
    // has at most four significant bits, i.e. nothing below the three bits under its top bit h.  NaN fits, +-inf does not (the
    // format has none).  Spelled out in integers, not through the hardware's rounding conversion: the rule is the wrapper's.
    static __device__ __forceinline__ bool fits(float x) {
        const float a = __builtin_fabsf(x);
        if (!(a <= 448.0f)) return x != x;
        const float t = a * 512.0f;
        const uint32_t u = static_cast<uint32_t>(t);
        const int h = 31 - __builtin_clz(u | 8u);          // >= 3
        return static_cast<float>(u) == t && (u & ((1u << (h - 3)) - 1u)) == 0;
    }
    // u < 8: a subnormal (or zero), E = 0 and M = u; else E = h - 2 and M = the three bits under the top one.  -0.0 keeps its sign.
    static __device__ __forceinline__ fsp_f8e4m3 narrow(float x) {
        const uint32_t u = static_cast<uint32_t>(__builtin_fabsf(x) * 512.0f);
        const int h = 31 - __builtin_clz(u | 8u);
        const uint32_t mag = u < 8u ? u : (static_cast<uint32_t>(h - 2) << 3) | ((u >> (h - 3)) & 7u);
        return fsp_f8e4m3{static_cast<uint8_t>(x != x ? 0x7fu : mag | ((__float_as_uint(x) >> 24) & 0x80u))};
    }
    static __device__ __forceinline__ bool fits(double x) { return RowCodec<float>::fits(x) && fits(static_cast<float>(x)); }
    static __device__ __forceinline__ fsp_f8e4m3 narrow(double x) { return narrow(static_cast<float>(x)); }
};

// every row of the table has its codec, and every codec fills a 16-byte slot
#define FSPANN_CODEC_CHECK(ID, T, QUERY, FINITE, WORDS, USES, NOUN) static_assert(sizeof(RowCodec<T>::slot) == 16 && RowCodec<T>::N * sizeof(T) == 16 && RowCodec<T>::always_finite == FINITE, #ID ": row codec");
FSPANN_DTYPE_TABLE(FSPANN_CODEC_CHECK)
#undef FSPANN_CODEC_CHECK

}  // namespace fspann
