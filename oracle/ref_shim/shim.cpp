/*
 * shim.cpp -- definitions behind ref_shim/ipp.h and ref_shim/mkl.h (TEST INFRASTRUCTURE, own text).
 *
 * THE RULE: a definition that returns data to the caller may never be added here.
 *
 * The reference build pins this project's oracle and kernels on the reference's own arithmetic.  A pin must not rest on
 * arithmetic written here, so this file holds exactly two kinds of definition:
 *   - the seven library start-up calls the reference's base constructor reaches (initialisation, a version string for
 *     its banner, thread counts): no-ops, none returns a number that enters a result;
 *   - every function that would compute (transposes, sgemv, omatcopy): prints its name and abort()s.  If a harness run
 *     ever ends here, a case was chosen wrongly: remove the case, not the abort.
 * The print_* / compare helpers are the debug printers that the reference's lib/simd_debug.h declares and its headers
 * include; no pinned path calls them, so they abort as well.
 */
#include <cstdio>
#include <cstdlib>
#include <string>

#include <immintrin.h>

#include "ipp.h"
#include "mkl.h"

static void not_pinned(const char *name) {
    std::fprintf(stderr, "ref_shim: %s was reached -- it is Intel library code, not the reference's own arithmetic, and is not "
                         "available here.  The case that called it cannot be pinned: remove the case.\n", name);
    std::abort();
}

extern "C" {

/* ---- start-up: no-ops ------------------------------------------------------------------------------------------- */
IppStatus ippInit(void) { return ippStsNoErr; }

const IppLibraryVersion *ippGetLibVersion(void) {
    static const IppLibraryVersion v = {"ref_shim (no Intel IPP: declarations only)", "0"};
    return &v;
}

IppStatus ippGetCpuFeatures(Ipp64u *mask, void *) {
    *mask = 0; /* banner only: every feature prints as N */
    return ippStsNoErr;
}

Ipp64u ippGetEnabledCpuFeatures(void) { return 0; }

IppStatus ippSetNumThreads(int) { return ippStsNoErr; }

void mkl_get_version_string(char *buf, int len) { std::snprintf(buf, (size_t)len, "ref_shim (no Intel MKL: declarations only)"); }

void mkl_set_num_threads(int) {}

/* ---- computing functions: abort --------------------------------------------------------------------------------- */
IppStatus ippiTranspose_8u_C1R(const Ipp8u *, int, Ipp8u *, int, IppiSize) { not_pinned("ippiTranspose_8u_C1R"); return 0; }
IppStatus ippiTranspose_16u_C1R(const Ipp16u *, int, Ipp16u *, int, IppiSize) { not_pinned("ippiTranspose_16u_C1R"); return 0; }
IppStatus ippiTranspose_32f_C1R(const Ipp32f *, int, Ipp32f *, int, IppiSize) { not_pinned("ippiTranspose_32f_C1R"); return 0; }

void cblas_sgemv(CBLAS_LAYOUT, CBLAS_TRANSPOSE, int, int, float, const float *, int, const float *, int, float, float *, int) {
    not_pinned("cblas_sgemv");
}

void mkl_somatcopy(char, char, size_t, size_t, float, const float *, size_t, float *, size_t) { not_pinned("mkl_somatcopy"); }

} /* extern "C" */

/* ---- lib/simd_debug.h: debug printers, never on a pinned path --------------------------------------------------- */
void print_epi8(__m256i) { not_pinned("print_epi8"); }
void print_epi16(__m256i) { not_pinned("print_epi16"); }
void print_epi32(__m256i) { not_pinned("print_epi32"); }
void print_ps(__m256) { not_pinned("print_ps"); }
std::string compare(std::string, std::string) { not_pinned("compare"); return std::string(); }
