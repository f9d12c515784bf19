// helm_client64.cpp — CPU key generation, encryption, decryption for the shortint
// (LUT / arithmetic mode) path: 64-bit torus, ciphertexts under the big key
// (include/helm_client.h).  Client-side counterpart of tfhe::shortint::{gen_keys,
// ClientKey} as HELM uses them (reference src/bin/helm.rs:301, src/circuit.rs:982-996,1092).
#include "../../include/helm_client.h"
#include "rng.hpp"

#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

namespace {

thread_local std::string g_err64;
int fail64(int code, const std::string &m)
{
    g_err64 = m;
    return code;
}

using Rng64 = helm_rng::Rng;

} // namespace

struct helm_si_client_key {
    helm_si_params P;
    double lwe_std, glwe_std;
    std::vector<uint64_t> lwe_sk, glwe_sk, bsk, ksk;
    uint64_t delta;
    Rng64 enc_rng;
};

extern "C" {

int helm_si_client_named_params(const char *name, helm_si_params *p, double *lwe_std, double *glwe_std)
{
    if (!name || !p || !lwe_std || !glwe_std) return fail64(HELM_ERR_INVALID, "null argument");
    std::memset(p, 0, sizeof(*p));
    const std::string s(name);
    p->k = 1;
    p->message_modulus = 4;
    p->carry_modulus = 4;
    if (s == "shortint_m2c2") {
        // tfhe 0.4 shortint PARAM_MESSAGE_2_CARRY_2_KS_PBS [recalled, SURVEY.md App. B]
        p->n = 742; p->N = 2048; p->pbs_l = 1; p->pbs_logB = 23; p->ks_l = 5; p->ks_logB = 3;
        *lwe_std = 0.000007069849454709433;
        *glwe_std = 0.00000000000000029403601535432533;
    } else if (s == "shortint_m2c2_pbs_ks") {
        // shortint_m2c2's shape for the bootstrap-first order (HELM_SI_CREATE_PBS_KS; tfhe's PARAM_MESSAGE_2_CARRY_2_PBS_KS):
        // k = 1, N = 2048, one PBS level of 23 bits [shape as shortint_m2c2; tfhe's own n, keyswitch decomposition and noise
        // for this set are NOT in the tree and not recalled: an approximate set, chosen here.  The order is not a parameter -
        // the set runs in either - but in order 0 a wire row carries the KEYSWITCH's noise, which every linear combination
        // amplifies before the next modulus switch, so m2c2's LWE side does not carry over: with n = 742, KS 5 x 3 the
        // formulas below give 2^-40.3 on a fresh output but 2^-13 on 2x + y and 2^-4.4 on 4x + 2y + z.  Taken: n = 840 with
        // the LWE noise on tfhe's security line through its n = 684 (2.04e-5) and n = 742 (7.07e-6) sets -
        // log2 sigma = -15.58 - 0.02643 (n - 684) = -19.70, sigma = 1.17e-6 - a keyswitch of 6 levels x 3 bits, and m2c2's
        // GLWE noise.  By the formulas of tests/test_gpu_noise.py (variances, torus units): blind rotation 2^-30.9,
        // keyswitch 2^-23.3 (the key's noise through the digits; the rounding term is 2^-29.6), modulus switch
        // (1 + n/2) / (48 N^2) = 2^-18.9.  A wire row holds blind rotation + keyswitch; the next look-up adds the modulus
        // switch; half a box is 1 / (4 t) = 2^-6.  Failure probability per look-up in order 0: 2^-84 on a fresh output
        // (variance br + ks + ms, sigma 2^-9.4), 2^-72 on 2x + y (5 (br + ks) + ms), 2^-46.5 on 4x + 2y + z of three
        // look-up outputs (21 (br + ks) + ms).  These are predictions of the formulas, not measured here]
        p->n = 840; p->N = 2048; p->pbs_l = 1; p->pbs_logB = 23; p->ks_l = 6; p->ks_logB = 3;
        *lwe_std = 0.000001172;
        *glwe_std = 0.00000000000000029403601535432533;
    } else if (s == "shortint_m2c2_multibit3") {
        // PARAM_MULTI_BIT_MESSAGE_2_CARRY_2_GROUP_3_KS_PBS, the set of reference src/bin/helm.rs:83
        // [dimensions recalled; noise: the LWE value extrapolated along tfhe's
        // security line through the n = 684 and n = 742 sets, the GLWE value of the N = 2048 sets]
        p->n = 888; p->N = 2048; p->pbs_l = 1; p->pbs_logB = 21; p->ks_l = 3; p->ks_logB = 4;
        p->grouping_factor = 3;
        *lwe_std = 0.00000049;
        *glwe_std = 0.00000000000000029403601535432533;
    } else if (s == "si_toy_2048_mb3") {
        p->n = 12; p->N = 2048; p->pbs_l = 1; p->pbs_logB = 21; p->ks_l = 3; p->ks_logB = 4;
        p->grouping_factor = 3;
        *lwe_std = 1e-9;
        *glwe_std = 1e-16;
    } else if (s == "shortint_m1c1") {
        // tfhe 0.4 shortint PARAM_MESSAGE_1_CARRY_1_KS_PBS, the set the reference binary installs for LUT mode
        // (src/bin/helm.rs:301) [dimensions recalled, SURVEY.md App. B: n = 684, k = 3, N = 512, PBS 18 x 1,
        // KS 4 x 3, message_modulus = carry_modulus = 2; LWE noise recalled; GLWE noise interpolated along tfhe's
        // security line between its k N = 1024 (4.99e-8) and k N = 2048 (2.94e-16) values: an approximate set]
        p->n = 684; p->k = 3; p->N = 512; p->pbs_l = 1; p->pbs_logB = 18; p->ks_l = 3; p->ks_logB = 4;
        p->message_modulus = 2; p->carry_modulus = 2;
        *lwe_std = 0.00002043357207216175;
        *glwe_std = 0.0000000000038;
    } else if (s == "shortint_m2c1") {
        // tfhe shortint PARAM_MESSAGE_2_CARRY_1_KS_PBS, the set of the reference's LUT-mode test (tests/circuit_test.rs:13):
        // k = 2, N = 1024, one PBS level, message_modulus = 4, carry_modulus = 2 [shape recalled; n, the decompositions and
        // both noise values recalled with LOW confidence - SURVEY.md App. B lists them as unknown.  Taken here: m2c2's LWE
        // side (n, sigma, KS 5 x 3) and PBS base, and tfhe's GLWE noise for k N = 2048, the same GLWE dimension as m2c2's.
        // The TFHE formulas of tests/test_gpu_noise.py give 2^-72 per look-up, 4x + 2y + z of three outputs included
        // (DESIGN.md 2): an approximate set]
        p->n = 742; p->k = 2; p->N = 1024; p->pbs_l = 1; p->pbs_logB = 23; p->ks_l = 5; p->ks_logB = 3;
        p->carry_modulus = 2;
        *lwe_std = 0.000007069849454709433;
        *glwe_std = 0.00000000000000029403601535432533;
    } else if (s == "si_toy_1024_k2") { // shortint_m2c1's shape at toy size (oracle-sized)
        p->n = 10; p->k = 2; p->N = 1024; p->pbs_l = 1; p->pbs_logB = 23; p->ks_l = 5; p->ks_logB = 3;
        p->carry_modulus = 2;
        *lwe_std = 1e-9;
        *glwe_std = 1e-15;
    } else if (s == "si_toy_512_k3") { // the k = 3 kernel at toy size (oracle-sized; 16 plaintext values like the other toys)
        p->n = 10; p->k = 3; p->N = 512; p->pbs_l = 1; p->pbs_logB = 18; p->ks_l = 3; p->ks_logB = 4;
        *lwe_std = 1e-9;
        *glwe_std = 1e-15;
    } else if (s == "si_toy_512_k2") {
        p->n = 9; p->k = 2; p->N = 512; p->pbs_l = 1; p->pbs_logB = 20; p->ks_l = 4; p->ks_logB = 3;
        *lwe_std = 1e-9;
        *glwe_std = 1e-15;
    } else if (s == "si_toy_1024_mb2") {
        p->n = 8; p->N = 1024; p->pbs_l = 1; p->pbs_logB = 22; p->ks_l = 5; p->ks_logB = 3;
        p->grouping_factor = 2;
        *lwe_std = 1e-9;
        *glwe_std = 1e-15;
    } else if (s == "shortint_m2c3") {
        // A 5-bit set, message_modulus 4 x carry_modulus 8 (tfhe's PARAM_MESSAGE_2_CARRY_3_KS_PBS): k = 1, N = 4096, one PBS
        // level of 22 bits [shape recalled; n, the keyswitch decomposition and both noise values are NOT recalled: an
        // approximate set, chosen as shortint_m2c1's were.  Taken here: n = 1024 (the engine's limit) with an LWE noise
        // extrapolated along tfhe's security line through its n = 684 (2.04e-5) and n = 742 (7.07e-6) sets -
        // log2 sigma = -15.58 - 0.02643 (n - 684) gives 2^-24.56 = 4.0e-8 - a keyswitch of 8 levels x 3 bits (the engine's
        // deepest), and tfhe's GLWE noise for N >= 4096, recalled as 2^-62 = 2.168e-19.
        // By the formulas of tests/test_gpu_noise.py (variances, torus units): blind rotation 2^-27.6 (all of it the
        // decomposition's rounding, n (1 + N/2) / (24 B^2): the key's noise through the digits is 2^-60.6), keyswitch 2^-31.7,
        // modulus switch (1 + n/2) / (48 N^2) = 2^-20.6 - the dominant term.  Half a box is 1 / (4 t) = 2^-7 at t = 32.
        // Failure probability per look-up: 2^-72 on one look-up output or a fresh encryption (sigma 2^-10.3: 9.8 standard
        // deviations), 2^-70 on a bivariate operand, 2^-63 on 4x + 2y + z of three outputs - and 2^-21.6 on
        // 16x + 8y + 4z + 2u + v of FIVE look-up outputs, where 341 x the blind rotation's rounding (2^-19.2) takes over: a
        // chain of 5-input gates wants a finer PBS decomposition than the recalled 22 x 1, which the capacity of the
        // kernel's pair stops at (23 x 1 is refused); 5-input gates on fresh inputs are at 2^-72]
        p->n = 1024; p->N = 4096; p->pbs_l = 1; p->pbs_logB = 22; p->ks_l = 8; p->ks_logB = 3;
        p->carry_modulus = 8;
        *lwe_std = 0.00000004;
        *glwe_std = 0.0000000000000000002168404344971009;
    } else if (s == "si_toy_4096") { // shortint_m2c3's shape at toy size (oracle-sized): 32 plaintext values
        p->n = 12; p->N = 4096; p->pbs_l = 1; p->pbs_logB = 22; p->ks_l = 3; p->ks_logB = 5;
        p->carry_modulus = 8;
        *lwe_std = 1e-9;
        *glwe_std = 1e-17;
    } else if (s == "shortint_m3c3") {
        // A 6-bit set, message_modulus 8 x carry_modulus 8 (tfhe's PARAM_MESSAGE_3_CARRY_3_KS_PBS): k = 1, N = 8192, PBS 15 x 2
        // (two levels of 15 bits), KS 3 x 6 (six levels of 3 bits), n = 864 [all recalled, none checked against tfhe's source:
        // an approximate set, like shortint_m2c3.  The LWE noise is not recalled: it is taken on tfhe's security line through
        // its n = 684 (2.04e-5) and n = 742 (7.07e-6) sets, log2 sigma = -15.58 - 0.02643 (n - 684) = -20.34, 7.55e-7; the
        // GLWE noise is tfhe's value for N >= 4096, recalled as 2^-62 = 2.168e-19.
        // By the formulas of tests/test_gpu_noise.py (variances, torus units): blind rotation 2^-42.8 (the decomposition's
        // rounding; the key's noise through the digits is 2^-72.8), keyswitch 2^-22.6 (the key's noise through the digits; the
        // rounding term is 2^-27.6), modulus switch (1 + n/2) / (48 N^2) = 2^-22.8.  Half a box is 1 / (4 t) = 2^-8 at t = 64.
        // Failure probability per look-up (variance weight x blind rotation + keyswitch + modulus switch: wires are big rows,
        // the operand is packed on them and keyswitched ONCE): 2^-40.7 on one look-up output or a fresh encryption (sigma
        // 2^-10.85: 7.2 standard deviations), and 2^-40.7 as well on a 6-input operand 32x + 16y + 8z + 4u + 2v + w of six
        // look-up outputs - the weight 1365 raises the blind rotation's term to 2^-32.4 only, far below the keyswitch and the
        // modulus switch, so a chain of 6-input gates costs no margin in this order.  (Under HELM_SI_CREATE_PBS_KS wires are
        // keyswitched rows and the keyswitch term would be weighted too: 1365 x 2^-22.6, which fails; this set is the KS_PBS
        // one.)  These are predictions of the formulas, not measured here]
        p->n = 864; p->N = 8192; p->pbs_l = 2; p->pbs_logB = 15; p->ks_l = 6; p->ks_logB = 3;
        p->message_modulus = 8; p->carry_modulus = 8;
        *lwe_std = 0.000000755;
        *glwe_std = 0.0000000000000000002168404344971009;
    } else if (s == "si_toy_8192") { // shortint_m3c3's shape at toy size (oracle-sized): 64 plaintext values
        p->n = 12; p->N = 8192; p->pbs_l = 2; p->pbs_logB = 15; p->ks_l = 3; p->ks_logB = 5;
        p->message_modulus = 8; p->carry_modulus = 8;
        *lwe_std = 1e-9;
        *glwe_std = 1e-17;
    } else if (s == "shortint_m3c3_multibit3") {
        // shortint_m3c3's values with grouping_factor = 3 (864 = 3 x 288 groups), for the multi-bit form of the N = 8192 kernel
        // (HELM_SI_CREATE_N8192 | HELM_SI_CREATE_LARGE_MULTIBIT) [an approximate set, as shortint_m3c3 is: tfhe's own
        // PARAM_MULTI_BIT_MESSAGE_3_CARRY_3_GROUP_3 values are not in the tree and not recalled.  PBS 15 x 2 loads at every
        // grouping factor: a generated key's group sums are near 2^94 against the pair's half of 2^97.87.
        // By the formulas of tests/test_gpu_noise.py with the multi-bit terms - per group 2^g x the key's noise through the
        // digits, and the rounding term with 12 in place of 24 over n / g groups: blind rotation 2^-43.4 (the rounding; the
        // key's noise through the digits is 2^-71.4, a factor 8 / 3 above the classical 2^-72.8), keyswitch 2^-22.6, modulus
        // switch 2^-22.8, unchanged.  Failure probability per look-up: 2^-40.7 on a fresh encryption or one look-up output,
        // and 2^-40.7 on the full-arity operand 32x + 16y + 8z + 4u + 2v + w of six look-up outputs (weight 1365 x 2^-43.4 =
        // 2^-33.0 stays far below the keyswitch and the modulus switch) - shortint_m3c3's figures: at this decomposition the
        // grouping costs no margin.  Predictions of the formulas, not measured here]
        p->n = 864; p->N = 8192; p->pbs_l = 2; p->pbs_logB = 15; p->ks_l = 6; p->ks_logB = 3;
        p->message_modulus = 8; p->carry_modulus = 8;
        p->grouping_factor = 3;
        *lwe_std = 0.000000755;
        *glwe_std = 0.0000000000000000002168404344971009;
    } else if (s == "shortint_m2c3_multibit3") {
        // shortint_m2c3's LWE side (keyswitch 8 x 3, LWE noise 4.0e-8; the security line gives 4.1e-8 at this n) with
        // n = 1023 = 3 x 341 groups, grouping_factor = 3 and PBS 15 x 2, for the multi-bit form of the large-N kernel
        // (HELM_SI_CREATE_LARGE_N | HELM_SI_CREATE_LARGE_MULTIBIT) [an approximate set.  The recalled 22 x 1 of shortint_m2c3
        // cannot load in multi-bit: a generated key's group sums would be near 2^(22 + 3 + 62 + 12) = 2^99, over the pair's
        // half of 2^97.87 (one level loads up to pbs_logB + grouping_factor = 23); 15 x 2 is at 2^93.
        // By the formulas of tests/test_gpu_noise.py with the multi-bit terms: blind rotation 2^-44.2 (the rounding; the key's
        // noise through the digits is 2^-72.2), keyswitch 2^-31.6, modulus switch 2^-20.6 - the dominant term, as in
        // shortint_m2c3.  Half a box is 2^-7 at t = 32.  Failure probability per look-up: 2^-72.8 on a fresh encryption or
        // one look-up output (9.8 standard deviations), and 2^-72.8 as well on the full-arity operand 16x + 8y + 4z + 2u + v
        // of five look-up outputs: the weight 341 raises the blind rotation's term to 2^-35.8 only - the finer decomposition
        // is what shortint_m2c3's comment asks for, where that operand is at 2^-21.6.  The formulas admit 15 x 2 at n = 1023,
        // so no other decomposition was looked for.  Predictions of the formulas, not measured here]
        p->n = 1023; p->N = 4096; p->pbs_l = 2; p->pbs_logB = 15; p->ks_l = 8; p->ks_logB = 3;
        p->carry_modulus = 8;
        p->grouping_factor = 3;
        *lwe_std = 0.00000004;
        *glwe_std = 0.0000000000000000002168404344971009;
    } else if (s == "si_toy_4096_mb2" || s == "si_toy_4096_mb3") {
        // si_toy_4096 for the multi-bit form of the large-N kernel (HELM_SI_CREATE_LARGE_MULTIBIT): n = 12 is divisible by
        // both grouping factors, and pbs_logB + grouping_factor = 23 is the largest a one-level key of this N loads with
        p->grouping_factor = s.back() - '0';
        p->n = 12; p->N = 4096; p->pbs_l = 1; p->pbs_logB = 23 - p->grouping_factor; p->ks_l = 3; p->ks_logB = 5;
        p->carry_modulus = 8;
        *lwe_std = 1e-9;
        *glwe_std = 1e-17;
    } else if (s == "si_toy_8192_mb2" || s == "si_toy_8192_mb3") {
        // si_toy_8192 for the multi-bit form of the N = 8192 kernel: PBS 15 x 2 loads at every grouping factor
        p->grouping_factor = s.back() - '0';
        p->n = 12; p->N = 8192; p->pbs_l = 2; p->pbs_logB = 15; p->ks_l = 3; p->ks_logB = 5;
        p->message_modulus = 8; p->carry_modulus = 8;
        *lwe_std = 1e-9;
        *glwe_std = 1e-17;
    } else if (s == "si_toy_512") {
        p->n = 12; p->N = 512; p->pbs_l = 2; p->pbs_logB = 15; p->ks_l = 4; p->ks_logB = 4;
        *lwe_std = 1e-9;
        *glwe_std = 1e-15;
    } else if (s == "si_toy_1024") {
        p->n = 10; p->N = 1024; p->pbs_l = 1; p->pbs_logB = 23; p->ks_l = 5; p->ks_logB = 3;
        *lwe_std = 1e-9;
        *glwe_std = 1e-15;
    } else if (s == "si_toy_2048") {
        p->n = 8; p->N = 2048; p->pbs_l = 1; p->pbs_logB = 23; p->ks_l = 5; p->ks_logB = 3;
        *lwe_std = 1e-9;
        *glwe_std = 1e-16;
    } else if (s == "si_toy_2048_l2") {
        p->n = 6; p->N = 2048; p->pbs_l = 2; p->pbs_logB = 14; p->ks_l = 3; p->ks_logB = 5;
        *lwe_std = 1e-9;
        *glwe_std = 1e-16;
    } else
        return fail64(HELM_ERR_INVALID, "unknown shortint parameter set '" + s + "'");
    return 0;
}

int helm_si_client_keygen(const helm_si_params *params, double lwe_std, double glwe_std, uint64_t seed,
                          helm_si_client_key **out)
{
    if (!params || !out) return fail64(HELM_ERR_INVALID, "null argument");
    *out = nullptr;
    const helm_si_params &P = *params;
    const int t = P.message_modulus * P.carry_modulus;
    if (P.n < 1 || P.k < 1 || P.N < 2 || (P.N & (P.N - 1)) || P.pbs_l < 1 || P.ks_l < 1 || P.pbs_logB < 1 ||
        P.ks_logB < 1 || P.pbs_logB * P.pbs_l > 64 || P.ks_logB * P.ks_l > 64 || t < 2 || (t & (t - 1)))
        return fail64(HELM_ERR_INVALID, "bad parameter set");
    const int g = P.grouping_factor > 1 ? P.grouping_factor : 1;
    if (g > 4 || P.n % g) return fail64(HELM_ERR_INVALID, "grouping_factor must be at most 4 and divide n");
    helm_si_client_key *K = new (std::nothrow) helm_si_client_key();
    if (!K) return fail64(HELM_ERR_OOM, "key");
    // seed 0: ChaCha20 streams under an OS-drawn key; otherwise the deterministic test generator (rng.hpp)
    std::unique_ptr<helm_rng::Source> src_p;
    try {
        src_p.reset(new helm_rng::Source(seed));
        K->enc_rng = src_p->encryption(0xE1C64);
    } catch (const std::exception &e) {
        delete K;
        return fail64(HELM_ERR_STATE, e.what());
    }
    const helm_rng::Source &src = *src_p;
    K->P = P;
    K->lwe_std = lwe_std;
    K->glwe_std = glwe_std;
    K->delta = (1ull << 63) / (uint64_t)t;
    const int n = P.n, k = P.k, N = P.N, k1 = k + 1, kN = k * N;
    Rng64 r0 = src.stream(0x51);
    K->lwe_sk.resize(n);
    for (auto &b : K->lwe_sk) b = r0.next() >> 63;
    K->glwe_sk.resize(kN);
    for (auto &b : K->glwe_sk) b = r0.next() >> 63;

    // ---- bootstrapping key, [n_ggsw][l][k+1 rows][k+1 polys][N] ---------------------------
    //      classical: GGSW(s_i) for every mask word; multi-bit: per group of g words the 2^g
    //      GGSWs of the subset indicators (bit i of the subset index = member i of the group)
    const size_t poly_per_i = (size_t)P.pbs_l * k1 * k1;
    const int subsets = g > 1 ? 1 << g : 1;
    const int n_ggsw = g > 1 ? (n / g) * subsets : n;
    K->bsk.assign((size_t)n_ggsw * poly_per_i * N, 0);
    #pragma omp parallel for schedule(dynamic, 4)
    for (int i = 0; i < n_ggsw; i++) {
        uint64_t message = 0;
        if (g > 1) {
            const int grp = i / subsets, S = i % subsets;
            message = 1;
            for (int q = 0; q < g; q++) message &= ((S >> q) & 1) ? K->lwe_sk[grp * g + q] : 1 - K->lwe_sk[grp * g + q];
        } else
            message = K->lwe_sk[i];
        Rng64 r = src.stream(0x6400000 + (uint64_t)i);
        std::vector<uint64_t> body(N);
        for (int j = 0; j < P.pbs_l; j++)
            for (int row = 0; row < k1; row++) {
                uint64_t *glwe = K->bsk.data() + (((size_t)i * P.pbs_l + j) * k1 + row) * k1 * N;
                for (int u = 0; u < N; u++) body[u] = r.noise64(glwe_std);
                for (int c = 0; c < k; c++) {
                    uint64_t *A = glwe + (size_t)c * N;
                    for (int u = 0; u < N; u++) A[u] = r.next();
                    const uint64_t *S = K->glwe_sk.data() + (size_t)c * N;
                    for (int u = 0; u < N; u++) {
                        if (!S[u]) continue;
                        for (int v = 0; v < N - u; v++) body[v + u] += A[v];
                        for (int v = N - u; v < N; v++) body[v + u - N] -= A[v];
                    }
                }
                std::memcpy(glwe + (size_t)k * N, body.data(), sizeof(uint64_t) * N);
                if (message) glwe[(size_t)row * N] += (uint64_t)1 << (64 - P.pbs_logB * (j + 1));
            }
    }
    // ---- keyswitching key: [k*N][ks_l][n+1] ---------------------------------------------
    K->ksk.assign((size_t)kN * P.ks_l * (n + 1), 0);
    #pragma omp parallel for schedule(dynamic, 16)
    for (int u = 0; u < kN; u++) {
        Rng64 r = src.stream(0x6500000 + (uint64_t)u);
        for (int j = 0; j < P.ks_l; j++) {
            uint64_t *ct = K->ksk.data() + ((size_t)u * P.ks_l + j) * (n + 1);
            uint64_t b = r.noise64(lwe_std);
            for (int i = 0; i < n; i++) {
                ct[i] = r.next();
                if (K->lwe_sk[i]) b += ct[i];
            }
            if (K->glwe_sk[u]) b += (uint64_t)1 << (64 - P.ks_logB * (j + 1));
            ct[n] = b;
        }
    }
    *out = K;
    return 0;
}

void helm_si_client_key_free(helm_si_client_key *key) { delete key; }

int helm_si_client_params(const helm_si_client_key *key, helm_si_params *out)
{
    if (!key || !out) return fail64(HELM_ERR_INVALID, "null argument");
    *out = key->P;
    return 0;
}
int helm_si_client_noise(const helm_si_client_key *key, double *lwe_noise_std, double *glwe_noise_std)
{
    if (!key || !lwe_noise_std || !glwe_noise_std) return fail64(HELM_ERR_INVALID, "null argument");
    *lwe_noise_std = key->lwe_std;
    *glwe_noise_std = key->glwe_std;
    return 0;
}

size_t helm_si_client_bsk_words(const helm_si_client_key *key) { return key ? key->bsk.size() : 0; }
size_t helm_si_client_ksk_words(const helm_si_client_key *key) { return key ? key->ksk.size() : 0; }
const uint64_t *helm_si_client_bsk(const helm_si_client_key *key) { return key ? key->bsk.data() : nullptr; }
const uint64_t *helm_si_client_ksk(const helm_si_client_key *key) { return key ? key->ksk.data() : nullptr; }
const uint64_t *helm_si_client_lwe_secret(const helm_si_client_key *key) { return key ? key->lwe_sk.data() : nullptr; }
const uint64_t *helm_si_client_glwe_secret(const helm_si_client_key *key) { return key ? key->glwe_sk.data() : nullptr; }

int helm_si_client_encrypt(helm_si_client_key *key, const uint64_t *values, int64_t count, uint64_t *out)
{
    if (!key || !values || !out || count < 0) return fail64(HELM_ERR_INVALID, "bad argument");
    const int dim = key->P.k * key->P.N;
    const uint64_t t = (uint64_t)key->P.message_modulus * key->P.carry_modulus;
    for (int64_t g = 0; g < count; g++) {
        uint64_t *ct = out + (size_t)g * (dim + 1);
        uint64_t b = key->enc_rng.noise64(key->glwe_std);
        for (int i = 0; i < dim; i++) {
            ct[i] = key->enc_rng.next();
            if (key->glwe_sk[i]) b += ct[i];
        }
        ct[dim] = b + (values[g] % t) * key->delta;
    }
    return 0;
}

// Rows of n + 1 words under the LWE key with the LWE noise: the wire rows of a context in the bootstrap-first order
// (HELM_SI_CREATE_PBS_KS; tfhe's EncryptionKeyChoice::Small).  The same encoding v * delta.
int helm_si_client_encrypt_small(helm_si_client_key *key, const uint64_t *values, int64_t count, uint64_t *out)
{
    if (!key || !values || !out || count < 0) return fail64(HELM_ERR_INVALID, "bad argument");
    const int n = key->P.n;
    const uint64_t t = (uint64_t)key->P.message_modulus * key->P.carry_modulus;
    for (int64_t g = 0; g < count; g++) {
        uint64_t *ct = out + (size_t)g * (n + 1);
        uint64_t b = key->enc_rng.noise64(key->lwe_std);
        for (int i = 0; i < n; i++) {
            ct[i] = key->enc_rng.next();
            if (key->lwe_sk[i]) b += ct[i];
        }
        ct[n] = b + (values[g] % t) * key->delta;
    }
    return 0;
}

int helm_si_client_phase(const helm_si_client_key *key, const uint64_t *lwe, int64_t count, int small, uint64_t *ph)
{
    if (!key || !lwe || !ph || count < 0) return fail64(HELM_ERR_INVALID, "bad argument");
    const int dim = small ? key->P.n : key->P.k * key->P.N;
    const uint64_t *sk = small ? key->lwe_sk.data() : key->glwe_sk.data();
    for (int64_t g = 0; g < count; g++) {
        const uint64_t *ct = lwe + (size_t)g * (dim + 1);
        uint64_t v = ct[dim];
        for (int i = 0; i < dim; i++)
            if (sk[i]) v -= ct[i];
        ph[g] = v;
    }
    return 0;
}

static int decrypt_rows(const helm_si_client_key *key, const uint64_t *lwe, int64_t count, int small, uint64_t *values)
{
    if (!key || !lwe || !values || count < 0) return fail64(HELM_ERR_INVALID, "bad argument");
    std::vector<uint64_t> ph((size_t)count);
    if (int rc = helm_si_client_phase(key, lwe, count, small, ph.data())) return rc;
    const uint64_t t = (uint64_t)key->P.message_modulus * key->P.carry_modulus;
    for (int64_t g = 0; g < count; g++) {
        // round to the nearest multiple of delta; the padding bit wraps into mod 2t, then mod t
        const uint64_t v = (ph[(size_t)g] + key->delta / 2) / key->delta;
        values[g] = v % t;
    }
    return 0;
}

int helm_si_client_decrypt(const helm_si_client_key *key, const uint64_t *lwe, int64_t count, uint64_t *values)
{
    return decrypt_rows(key, lwe, count, 0, values);
}

int helm_si_client_decrypt_small(const helm_si_client_key *key, const uint64_t *lwe, int64_t count, uint64_t *values)
{
    return decrypt_rows(key, lwe, count, 1, values);
}

} // extern "C"
