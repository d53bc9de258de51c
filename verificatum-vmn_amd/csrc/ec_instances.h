// ec_instances.h — the curve kernels of one field size as explicit instantiations (see modp_instances.h: the host unit
// vmnhip.hip declares them `extern template`, csrc/inst_p224.hip / inst_p256.hip / inst_p384.hip / inst_p521.hip (EC_NIST) and
// inst_g9.hip / inst_g10.hip / inst_g13.hip / inst_g15.hip / inst_g21.hip (EC_GENERAL) define them, compiled side by side).
#pragma once
#include "ec_kernels.h"

#define VMN_EC_INSTANCES(KW, S_, NW_, K_)                                                                                                 \
    KW __global__ void vmn::k_ec_import<S_, NW_, K_>(vmn::u32*, const uint8_t*, size_t, size_t, int, size_t, vmn::ECDev, vmn::u32*);     \
    KW __global__ void vmn::k_ec_export<S_, NW_, K_>(uint8_t*, size_t, size_t, int, const vmn::u32*, size_t, vmn::ECDev);                \
    KW __global__ void vmn::k_ec_add<S_, K_>(vmn::u32*, const vmn::u32*, const vmn::u32*, size_t, size_t, vmn::ECDev);                   \
    KW __global__ void vmn::k_ec_neg<S_, K_>(vmn::u32*, const vmn::u32*, size_t, vmn::ECDev);                                            \
    KW __global__ void vmn::k_ec_equal<S_, K_>(const vmn::u32*, const vmn::u32*, size_t, vmn::ECDev, vmn::u32*);                         \
    KW __global__ void vmn::k_ec_mulvar<S_, K_>(vmn::u32*, const vmn::u32*, const vmn::u32*, int, size_t, int, int, size_t, vmn::ECDev,  \
                                            vmn::u32*);                                                                                 \
    KW __global__ void vmn::k_ec_mulvar2<S_, K_>(vmn::u32*, const vmn::u32*, const vmn::u32*, int, int, const vmn::u32*, const vmn::u32*, int, \
                                             size_t, int, int, size_t, vmn::ECDev, vmn::u32*);                                          \
    KW __global__ void vmn::k_ec_expprod<S_, K_>(vmn::u32*, vmn::ECExpProdArrays, const vmn::SlideStep*, int, size_t, vmn::ECDev, vmn::u32*); \
    KW __global__ void vmn::k_ec_mulshared<S_, K_, vmn::ECOneArray>(vmn::ECOneArray, vmn::u32, vmn::u32, const vmn::ECSharedStep*, int, int, \
                                                                    size_t, vmn::ECDev, vmn::u32*);                                     \
    KW __global__ void vmn::k_ec_mulshared<S_, K_, vmn::ECSharedArrays>(vmn::ECSharedArrays, vmn::u32, vmn::u32, const vmn::ECSharedStep*, int, \
                                                                        int, size_t, vmn::ECDev, vmn::u32*);                            \
    KW __global__ void vmn::k_ec_mulshared<S_, K_, vmn::ECEachArrays>(vmn::ECEachArrays, vmn::u32, vmn::u32, const vmn::ECSharedStep*, int, int, \
                                                                      size_t, vmn::ECDev, vmn::u32*);                                   \
    KW __global__ void vmn::k_ec_chain<S_, K_>(vmn::u32*, const vmn::u32*, int, vmn::ECDev);                                             \
    KW __global__ void vmn::k_ec_fixed_level<S_, K_>(vmn::u32*, int, int, int, vmn::ECDev);                                              \
    KW __global__ void vmn::k_ec_fixed_exp<S_, K_>(vmn::u32*, const vmn::u32*, int, int, const vmn::u32*, int, size_t, vmn::ECDev);      \
    KW __global__ void vmn::k_finv_up<S_, true, K_>(vmn::u32*, vmn::u32*, vmn::LevelInputs, unsigned, size_t, size_t, vmn::ECDev);       \
    KW __global__ void vmn::k_finv_up<S_, false, K_>(vmn::u32*, vmn::u32*, vmn::LevelInputs, unsigned, size_t, size_t, vmn::ECDev);      \
    KW __global__ void vmn::k_finv_top<S_, K_>(vmn::u32*, const vmn::u32*, size_t, vmn::ECDev);                                          \
    KW __global__ void vmn::k_finv_down<S_, K_>(vmn::u32*, const vmn::u32*, const vmn::u32*, const vmn::u32*, size_t, size_t, vmn::ECDev); \
    KW __global__ void vmn::k_ec_normalize_down<S_, K_>(vmn::u32*, vmn::LevelInputs, unsigned, const vmn::u32*, const vmn::u32*, size_t, \
                                                    size_t, vmn::ECDev);                                                                \
    KW __global__ void vmn::k_ec_bucket_level<S_, true, K_>(vmn::u32*, size_t, vmn::LevelInputs, unsigned, const vmn::u32*, const vmn::u32*, \
                                                        const vmn::u32*, const vmn::u32*, size_t, size_t, vmn::u32, vmn::ECDev);        \
    KW __global__ void vmn::k_ec_bucket_level<S_, false, K_>(vmn::u32*, size_t, vmn::LevelInputs, unsigned, const vmn::u32*, const vmn::u32*, \
                                                         const vmn::u32*, const vmn::u32*, size_t, size_t, vmn::u32, vmn::ECDev);       \
    KW __global__ void vmn::k_ec_bucket_first_jacobian<S_, K_>(vmn::u32*, size_t, vmn::LevelInputs, unsigned, const vmn::u32*, const vmn::u32*, \
                                                           const vmn::u32*, const vmn::u32*, size_t, size_t, vmn::u32, vmn::ECDev);     \
    KW __global__ void vmn::k_ec_reduce<S_, K_>(vmn::u32*, const vmn::u32*, size_t, size_t, size_t, vmn::ECDev);                         \
    KW __global__ void vmn::k_ec_scan_totals<S_, K_>(vmn::u32*, const vmn::u32*, size_t, size_t, size_t, int, vmn::ECDev);               \
    KW __global__ void vmn::k_ec_scan_apply<S_, K_>(vmn::u32*, const vmn::u32*, const vmn::u32*, size_t, size_t, size_t, int, vmn::ECDev); \
    KW __global__ void vmn::k_ec_horner<S_, K_>(vmn::u32*, const vmn::u32*, int, int, int, vmn::ECDev);

// the NIST kind (a = -3; P-192 and prime192v2 / v3 run on the 9-limb kernels of P-224, which take their prime at run time)
#define VMN_UNIT_P224(KW) VMN_EC_INSTANCES(KW, 9, 7, vmn::EC_NIST)
#define VMN_UNIT_P256(KW) VMN_EC_INSTANCES(KW, 10, 8, vmn::EC_NIST)
#define VMN_UNIT_P384(KW) VMN_EC_INSTANCES(KW, 15, 12, vmn::EC_NIST)
#define VMN_UNIT_P521(KW) VMN_EC_INSTANCES(KW, 21, 17, vmn::EC_NIST)
// the general kind (any a, any prime; csrc/inst_g*.hip): limb counts with R / p >= 2^24 and FW > S (ECfg)
#define VMN_UNIT_G9(KW) VMN_EC_INSTANCES(KW, 9, 7, vmn::EC_GENERAL)      // 192 / 224 bits: brainpoolp192r1 / p224r1, secp192k1 / p224k1
#define VMN_UNIT_G10(KW) VMN_EC_INSTANCES(KW, 10, 8, vmn::EC_GENERAL)    // 239 / 256 bits: prime239v1-3, brainpoolp256r1, secp256k1
#define VMN_UNIT_G13(KW) VMN_EC_INSTANCES(KW, 13, 10, vmn::EC_GENERAL)   // 320 bits: brainpoolp320r1
#define VMN_UNIT_G15(KW) VMN_EC_INSTANCES(KW, 15, 12, vmn::EC_GENERAL)   // 384 bits: brainpoolp384r1
#define VMN_UNIT_G21(KW) VMN_EC_INSTANCES(KW, 21, 17, vmn::EC_GENERAL)   // 512 bits: brainpoolp512r1
