// dtypes.h — what the library knows about each FSPANN_* dtype of include/fspann.h, in ONE table, and the two dispatchers that
// turn a dtype given at run time into a type tag.  Included from fspann_common.h behind the element types.  Every entry point
// goes through here: a new row type adds a row to the table and its RowCodec (row_codec.hip.h: how the kernels read an element; a
// static_assert there asks for one per row), and touches no dispatch site and no kernel.
#pragma once

namespace fspann {

// One row per dtype:
//   id, element type, may be a query dtype, every element is finite,
//   the words of its "row dtype only" refusal (null: not refused by name) and what that refusal lists behind "Setup input, ",
//   the noun of fspann_refine's refusal (null: fspann_refine takes it)
#define FSPANN_DTYPE_TABLE(X)                                                                                                      \
    X(FSPANN_F32, float, true, false, nullptr, nullptr, nullptr)                                                                   \
    X(FSPANN_F64, double, true, false, nullptr, nullptr, nullptr)                                                                  \
    X(FSPANN_U8, uint8_t, false, true, nullptr, nullptr, "byte rows")                                                              \
    X(FSPANN_F16, _Float16, false, false, "half precision", "metrics base", "half rows")                                           \
    X(FSPANN_BF16, fsp_bf16, false, false, "bfloat16", "metrics base", "bfloat16 rows")                                            \
    X(FSPANN_F8E4M3, fsp_f8e4m3, false, false, "fp8 e4m3fn", "metrics base", "fp8 rows")                                           \
    X(FSPANN_I8, int8_t, false, true, "signed int8", "metrics and ground truth over int8 pairs", "signed byte rows")

struct DtypeInfo {
    int id;
    const char* name;         // "FSPANN_F16"
    size_t size;              // bytes per element
    bool query;               // a query may have it (FSPANN_F32 and FSPANN_F64 only)
    bool finite;              // every element is finite (the byte types)
    const char* words;        // "half precision"
    const char* row_uses;     // "metrics base"
    const char* rows_noun;    // "half rows"
};
#define FSPANN_DTYPE_ROW(ID, T, QUERY, FINITE, WORDS, USES, NOUN) {ID, #ID, sizeof(T), QUERY, FINITE, WORDS, USES, NOUN},
constexpr DtypeInfo kDtypes[] = {FSPANN_DTYPE_TABLE(FSPANN_DTYPE_ROW)};
#undef FSPANN_DTYPE_ROW

// the table's row of a dtype; null: not a dtype of include/fspann.h
inline const DtypeInfo* dtype_info(int dtype) {
    for (const DtypeInfo& r : kDtypes)
        if (r.id == dtype) return &r;
    return nullptr;
}
// bytes per element (the callers have checked which dtypes they take; 4 for what is none)
inline size_t dtype_size(int dtype) {
    const DtypeInfo* r = dtype_info(dtype);
    return r ? r->size : 4;
}
// the row dtypes: what fspann_store_set / _attach_dev, fspann_build_index / _append and the rows of a refinement take (every dtype is one)
inline bool is_row_dtype(int dtype) { return dtype_info(dtype) != nullptr; }
inline bool is_query_dtype(int dtype) {
    const DtypeInfo* r = dtype_info(dtype);
    return r && r->query;
}
inline const char* dtype_name(int dtype) {
    const DtypeInfo* r = dtype_info(dtype);
    return r ? r->name : "unknown dtype";
}
// A row-only dtype given where none can stand (a query, the point store): refused by name, `what` being the argument.  FSPANN_OK
// for every other value: FSPANN_U8 and unknown numbers get the caller's own message.
inline int refuse_row_only(int dtype, const char* what) {
    const DtypeInfo* r = dtype_info(dtype);
    if (!r || !r->words) return FSPANN_OK;
    return fail(FSPANN_E_ARG, "%s %s: %s is a row dtype only (store, refine rows, Setup input, %s); this one is FSPANN_F32 or FSPANN_F64", what, r->name, r->words,
                r->row_uses);
}

// element type -> its row of the table, at compile time
template <typename T> struct DtypeOf;
#define FSPANN_DTYPE_OF(ID, T, QUERY, FINITE, WORDS, USES, NOUN) \
    template <> struct DtypeOf<T> { static constexpr int id = ID; static constexpr bool query = QUERY, finite = FINITE; };
FSPANN_DTYPE_TABLE(FSPANN_DTYPE_OF)
#undef FSPANN_DTYPE_OF

template <typename T> struct DtypeTag { using type = T; };
template <bool TAKE, typename T, class F> bool dtype_call_if(F& f) {
    if constexpr (TAKE) f(DtypeTag<T>{});
    return TAKE;
}
// f(DtypeTag<element type>{}) for the row dtype given at run time.  false: not a row dtype, f was not called (the caller words the error).
template <class F> bool with_row_type(int dtype, F&& f) {
    switch (dtype) {
#define FSPANN_DTYPE_CASE(ID, T, QUERY, FINITE, WORDS, USES, NOUN) case ID: return dtype_call_if<true, T>(f);
        FSPANN_DTYPE_TABLE(FSPANN_DTYPE_CASE)
#undef FSPANN_DTYPE_CASE
    default: return false;
    }
}
// the same over the query dtypes (f is instantiated for those only)
template <class F> bool with_query_type(int dtype, F&& f) {
    switch (dtype) {
#define FSPANN_DTYPE_CASE(ID, T, QUERY, FINITE, WORDS, USES, NOUN) case ID: return dtype_call_if<QUERY, T>(f);
        FSPANN_DTYPE_TABLE(FSPANN_DTYPE_CASE)
#undef FSPANN_DTYPE_CASE
    default: return false;
    }
}

}  // namespace fspann
