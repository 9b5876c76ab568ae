// dtype_table_check.cpp — the dtype table of csrc/dtypes.h as plain host code (tests/test_dtype_table_cpu.py builds it with
// AddressSanitizer + UBSan and runs it; no device is touched).  Every dtype id from -2 to 80 goes through the size, name, is-row and
// is-query lookups, the two dispatchers and the refusal by name; each answer is compared with the values written out here.
#include "../../fspann-query-system_amd/csrc/fspann_common.h"

#include <cstdio>
#include <cstring>

namespace {

struct Want {
    int id;
    const char* name;
    size_t size;
    bool query;
    const char* refusal;      // of refuse_row_only(id, "q_dtype"); null: not refused by name
};
const Want kWant[] = {
    {0, "FSPANN_F32", 4, true, nullptr},
    {1, "FSPANN_F64", 8, true, nullptr},
    {2, "FSPANN_U8", 1, false, nullptr},
    {3, "FSPANN_F16", 2, false,
     "q_dtype FSPANN_F16: half precision is a row dtype only (store, refine rows, Setup input, metrics base); this one is FSPANN_F32 or FSPANN_F64"},
    {4, "FSPANN_BF16", 2, false,
     "q_dtype FSPANN_BF16: bfloat16 is a row dtype only (store, refine rows, Setup input, metrics base); this one is FSPANN_F32 or FSPANN_F64"},
    {5, "FSPANN_F8E4M3", 1, false,
     "q_dtype FSPANN_F8E4M3: fp8 e4m3fn is a row dtype only (store, refine rows, Setup input, metrics base); this one is FSPANN_F32 or FSPANN_F64"},
    {6, "FSPANN_I8", 1, false,
     "q_dtype FSPANN_I8: signed int8 is a row dtype only (store, refine rows, Setup input, metrics and ground truth over int8 pairs); this one is FSPANN_F32 or "
     "FSPANN_F64"},
};

int bad = 0;
void expect(bool ok, int id, const char* what) {
    if (!ok) { std::printf("dtype %d: %s\n", id, what); bad++; }
}

}  // namespace

int main() {
    using namespace fspann;
    for (int id = -2; id <= 80; id++) {
        const Want* w = nullptr;
        for (const Want& x : kWant)
            if (x.id == id) w = &x;
        expect(is_row_dtype(id) == (w != nullptr), id, "is_row_dtype");
        expect(is_query_dtype(id) == (w && w->query), id, "is_query_dtype");
        expect(dtype_size(id) == (w ? w->size : 4), id, "dtype_size");
        expect(std::strcmp(dtype_name(id), w ? w->name : "unknown dtype") == 0, id, "dtype_name");
        // the dispatchers call back with the element type of this very id, or not at all
        size_t row_size = 0, q_size = 0;
        int row_id = -99, q_id = -99;
        const bool row = with_row_type(id, [&](auto t) { using T = typename decltype(t)::type; row_size = sizeof(T); row_id = DtypeOf<T>::id; });
        const bool qry = with_query_type(id, [&](auto t) { using T = typename decltype(t)::type; q_size = sizeof(T); q_id = DtypeOf<T>::id; });
        expect(row == (w != nullptr) && row_size == (w ? w->size : 0) && row_id == (w ? id : -99), id, "with_row_type");
        expect(qry == (w && w->query) && q_size == (qry ? w->size : 0) && q_id == (qry ? id : -99), id, "with_query_type");
        // the refusal: FSPANN_E_ARG and the whole message, or FSPANN_OK with the last error left alone
        last_error_ref() = "untouched";
        const int rc = refuse_row_only(id, "q_dtype");
        if (w && w->refusal) expect(rc == FSPANN_E_ARG && last_error_ref() == w->refusal, id, "refuse_row_only (message)");
        else expect(rc == FSPANN_OK && last_error_ref() == "untouched", id, "refuse_row_only (not refused)");
    }
    std::printf("dtype table: %d ids checked, %d wrong\n", 80 - (-2) + 1, bad);
    return bad ? 1 : 0;
}
