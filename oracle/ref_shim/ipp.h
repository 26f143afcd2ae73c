/*
 * ipp.h -- declarations only (TEST INFRASTRUCTURE, own text).
 *
 * The reference's include/CloverBase.h includes "ipp.h" and "mkl.h" unconditionally.  This header declares the names its
 * container headers mention, collected from the compiler's list of missing identifiers, so that those headers compile
 * where Intel IPP is not installed.  It contains no arithmetic.  The definitions live in shim.cpp: the start-up calls
 * are no-ops, every function that would compute aborts.
 */
#ifndef CLOVER_REF_SHIM_IPP_H
#define CLOVER_REF_SHIM_IPP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef unsigned char Ipp8u;
typedef unsigned short Ipp16u;
typedef float Ipp32f;
typedef unsigned long long Ipp64u;
typedef int IppStatus;

enum { ippStsNoErr = 0 };

typedef struct {
    int width;
    int height;
} IppiSize;

typedef struct {
    const char *Name;
    const char *Version;
} IppLibraryVersion;

/* feature bits: only printed as Y/N in the start-up banner; distinct bits, otherwise arbitrary */
enum {
    ippCPUID_MMX = 1 << 0,
    ippCPUID_SSE = 1 << 1,
    ippCPUID_SSE2 = 1 << 2,
    ippCPUID_SSE3 = 1 << 3,
    ippCPUID_SSSE3 = 1 << 4,
    ippCPUID_MOVBE = 1 << 5,
    ippCPUID_SSE41 = 1 << 6,
    ippCPUID_SSE42 = 1 << 7,
    ippCPUID_AVX = 1 << 8,
    ippAVX_ENABLEDBYOS = 1 << 9,
    ippCPUID_AES = 1 << 10,
    ippCPUID_CLMUL = 1 << 11,
    ippCPUID_RDRAND = 1 << 12,
    ippCPUID_F16C = 1 << 13,
    ippCPUID_AVX2 = 1 << 14,
    ippCPUID_ADCOX = 1 << 15,
    ippCPUID_RDSEED = 1 << 16,
    ippCPUID_PREFETCHW = 1 << 17,
    ippCPUID_SHA = 1 << 18,
    ippCPUID_AVX512F = 1 << 19,
    ippCPUID_AVX512CD = 1 << 20,
    ippCPUID_AVX512ER = 1 << 21,
    ippCPUID_KNC = 1 << 22
};

/* library start-up (shim.cpp: no-ops) */
IppStatus ippInit(void);
const IppLibraryVersion *ippGetLibVersion(void);
IppStatus ippGetCpuFeatures(Ipp64u *mask, void *cpuid_regs);
Ipp64u ippGetEnabledCpuFeatures(void);
IppStatus ippSetNumThreads(int n);

/* computing functions (shim.cpp: abort) */
IppStatus ippiTranspose_8u_C1R(const Ipp8u *src, int src_step, Ipp8u *dst, int dst_step, IppiSize roi);
IppStatus ippiTranspose_16u_C1R(const Ipp16u *src, int src_step, Ipp16u *dst, int dst_step, IppiSize roi);
IppStatus ippiTranspose_32f_C1R(const Ipp32f *src, int src_step, Ipp32f *dst, int dst_step, IppiSize roi);

#ifdef __cplusplus
}
#endif

#endif /* CLOVER_REF_SHIM_IPP_H */
