// api_dataset.cpp — the entry points of data set assembly (include/pmp.h): one index of the rows a set keeps, any array gathered by it.
// What they refuse is train_check.h's select_refused and rows_gather_refused; the kernels are dataset.hip's.
#include "pmp_host.h"
#include "train_check.h"

using namespace pmp;

// As the training calls: nothing is launched or written before the checks pass, then whatever is in flight on the context is made final
static int admit(pmp_ctx *c, const char *fn, const char *why)
{
    CHECK_CTX(c);
    if (why) return set_err(c, PMP_E_INVALID, std::string(fn) + ": " + why);
    return settle_before_host_call(c);
}

extern "C" {

int pmp_select_rows_device(pmp_ctx *c, const uint8_t *const *d_flags, int nflags, int mask, const int64_t *d_seg_end, int nseg, int64_t cap,
                           int64_t n, int64_t *d_index, int64_t *d_count)
{
    if (int rc = admit(c, "pmp_select_rows_device", select_refused(d_flags, nflags, mask, d_seg_end, nseg, cap, n, d_index, d_count))) return rc;
    if (int rc = ensure(c, c->d_select, select_scratch_words(n, nseg) * sizeof(uint32_t))) return rc;
    SelectFlags f{};
    for (int k = 0; k < nflags; ++k) f.p[k] = d_flags[k];
    const hipError_t e = launch_select_rows(c->stream, f, nflags, mask, d_seg_end, nseg, cap, n, (uint32_t *)c->d_select.p, d_index, d_count);
    return e == hipSuccess ? PMP_OK : hip_fail(c, e, "select_rows");
}

int pmp_gather_rows_device(pmp_ctx *c, const void *d_src, int64_t nsrc, int64_t row_bytes, const int64_t *d_index, int64_t m, void *d_dst,
                           int32_t *d_status)
{
    if (int rc = admit(c, "pmp_gather_rows_device", rows_gather_refused(d_src, nsrc, row_bytes, d_index, m, d_dst, d_status))) return rc;
    const hipError_t e = launch_gather_rows(c->stream, d_src, nsrc, row_bytes, d_index, m, d_dst, d_status);
    return e == hipSuccess ? PMP_OK : hip_fail(c, e, "gather_rows");
}

}  // extern "C"
