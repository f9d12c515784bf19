/*
 * helm_shortint.h — C ABI of the MI355X-native LUT-mode / arithmetic-mode engine
 * (64-bit torus, "shortint" ciphertexts: message + carry bits under one padding bit).
 *
 * Reference interfaces this replaces (all arithmetic inside the `tfhe` 0.4.1 crate,
 * Cargo.toml:18, absent from the tree):
 *   src/gates.rs:754-785      gates::lut(): tfhe::shortint::ServerKey::
 *                             {smart_evaluate_bivariate_function, smart_neg,
 *                              smart_scalar_left_shift, add, create_trivial,
 *                              generate_lookup_table, apply_lookup_table}
 *   src/circuit.rs:1032-1083  LutCircuit::evaluate_encrypted: per level,
 *                             gates.par_iter_mut() -> one lut() per gate
 *   src/circuit.rs:970-1000   encrypt_inputs (client_key.encrypt(u64), create_trivial(0))
 *   src/gates.rs:306-702      arithmetic-mode operators (FheUint8..128 = radix of shortint
 *                             blocks): served by the same two device primitives below
 *
 * Shape of the replacement.  Ciphertexts live in a device-resident table of "big" LWE
 * rows (k*N mask words + body, uint64) - tfhe's KS_PBS order: apply_lookup_table =
 * keyswitch big->small, then programmable bootstrap small->big.  Two level-batched
 * primitives carry every operator of both modes:
 *   helm_si_lincomb()      out = sum_t coef[t] * in[t] + const        (no bootstrap)
 *   helm_si_apply_luts()   out = PBS_lut( KS( in ) )                  (one bootstrap)
 * and helm_si_eval_lut_level() is gates::lut() for a whole netlist level.
 *
 * Conventions as in helm_hip.h: 0 / negative helm_status, helm_hip_last_error(),
 * caller owns host buffers, one context per device + host thread (several threads may share a
 * context if they serialise their calls - the host library's round merger does, under one lock),
 * stream-asynchronous with helm_si_sync(), no CPU fallback.
 *
 * Layouts (all words uint64_t, arithmetic mod 2^64)
 *   big LWE row          k*N mask words + body: the wire row of a context in order 1 (the default)
 *   small LWE row        n mask words + body: the wire row under HELM_SI_CREATE_PBS_KS (helm_si_wire_words)
 *   bootstrapping key    [n][pbs_l][k+1][k+1][N]      (as helm_hip.h, 64-bit); multi-bit sets
 *                        (grouping_factor g > 1): [n/g][2^g][pbs_l][k+1][k+1][N]
 *   keyswitching key     [k*N][ks_l][n+1]
 *   encoding             value v in [0, message_modulus*carry_modulus) -> v * delta,
 *                        delta = 2^63 / (message_modulus * carry_modulus)
 *                        (the one citable line: src/gates.rs:851)
 *   look-up table        test polynomial of N words: box v of N/(msg*carry) coefficients
 *                        = f(v) * delta, rotated left by half a box, wrapped part negated
 */
#ifndef HELM_SHORTINT_H
#define HELM_SHORTINT_H

#include <stddef.h>
#include <stdint.h>
#include "helm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct helm_si_ctx helm_si_ctx;
typedef struct helm_si_wires helm_si_wires;

/* tfhe::shortint::{ClassicPBSParameters, MultiBitPBSParameters} as HELM picks them
 * (src/bin/helm.rs:301, tests/circuit_test.rs:287; src/bin/helm.rs:83 for arithmetic mode),
 * runtime values.
 * grouping_factor g: 0 or 1 = classical blind rotation (n CMUX steps, key = GGSW(s_i));
 * g = 2 or 3 = multi-bit blind rotation (tfhe's MultiBitPBS, reference helm.rs:83 uses g = 3):
 * n/g group steps; the key holds, per group, 2^g GGSWs of the indicators
 * prod_{i in S} s_i * prod_{i not in S} (1 - s_i), S a subset of the group (bit i of the subset
 * index = member i), and a step is acc <- (sum_S X^(sum_{i in S} a~_i) * GGSW_S) (x) acc.
 * n must be a multiple of g.
 * Accepted: pbs_logB <= 24 and pbs_logB * pbs_l <= 31 (every tfhe shortint set; the kernels multiply decomposition digits by
 * a 25-bit root of unity without a modular reduction), exact products below the CRT pair's range (2^97.5). */
typedef struct {
    int32_t n, k, N;
    int32_t pbs_l, pbs_logB;
    int32_t ks_l, ks_logB;
    int32_t message_modulus, carry_modulus;
    int32_t grouping_factor;
} helm_si_params;

/* Replaces shortint ServerKey construction (helm.rs:301: gen_keys(PARAM_...)).  Admits the shapes the tuned bootstrap
 * builds cover: k = 1 at N in {512, 1024, 2048} with pbs_l in {1, 2}; k in {2, 3} at N = 512 and k = 2 at N = 1024, with
 * pbs_l = 1.  Equal to helm_si_ctx_create_ex(device_id, params, 0, out). */
int helm_si_ctx_create(int device_id, const helm_si_params *params, helm_si_ctx **out);

/* Flags of helm_si_ctx_create_ex. */
enum {
    HELM_SI_CREATE_ALLOW_GENERIC = 1, /* admit shapes no tuned build covers: they run on the generic kernel */
    HELM_SI_CREATE_FORCE_GENERIC = 2, /* run every launch on the generic kernel, tuned shapes too (implies 1) */
    /* 4 and 8 are reserved: refused as unknown bits */
    HELM_SI_CREATE_GENERIC_MULTIBIT = 16, /* with 1 or 2: multi-bit shapes may run on the generic kernel's multi-bit form */
    HELM_SI_CREATE_LARGE_N = 32, /* admit k = 1, N = 4096 (the 5-bit shortint sets): it runs on the large-N kernel */
    HELM_SI_CREATE_PBS_KS = 64, /* bootstrap-first order (tfhe's *_PBS_KS sets): wire rows of n + 1 words under the small key */
    /* 128 is not assigned: refused as an unknown bit */
    HELM_SI_CREATE_N8192 = 256, /* admit k = 1, N = 8192 (the 6-bit shortint sets): it runs on the N = 8192 kernel */
    /* 512 is not assigned: refused as an unknown bit */
    HELM_SI_CREATE_LARGE_MULTIBIT = 1024 /* with 32 and/or 256: multi-bit shapes at N = 4096 / 8192 run on those kernels */
};
/* helm_si_ctx_create with flags.  flags = 0 is helm_si_ctx_create: the same checks in the same order, the same messages.
 * With either flag, a shape no tuned build covers is admitted when it lies in the generic kernel's domain - N in {256, 512,
 * 1024, 2048} (FpG2 has 2-adicity 2^12: no 2N-th root of unity beyond N = 2048), k >= 1 with (k+1) N <= 4096 (the kernel's
 * LDS budget), pbs_l >= 1, grouping_factor <= 1 - and passes every other check of helm_si_ctx_create (n, the decompositions,
 * message_modulus * carry_modulus, the two-prime capacity bound).  Its bootstraps then run on k_pbs64_generic (k, pbs_l and
 * pbs_logB at run time, one workgroup per bootstrap, the 49-bit pair: helm_si_field_bits() returns 49).  Multi-bit shapes
 * without a tuned build are refused, and so is HELM_SI_CREATE_FORCE_GENERIC with grouping_factor > 1, unless
 * HELM_SI_CREATE_GENERIC_MULTIBIT is given (below).  Everything above
 * the bootstrap kernel (keyswitch, lincomb, look-up levels, lanes, audit, sharding, round capacity) works unchanged; the
 * WoP-PBS path (helm_wop_ctx_create) refuses a PBS-side context whose launches run generic.  An importer that meets a key
 * of an unfamiliar shape passes HELM_SI_CREATE_ALLOW_GENERIC on purpose: the generic kernel is slower than a tuned build.
 * HELM_SI_CREATE_GENERIC_MULTIBIT (only together with one of the two flags above; alone it is HELM_ERR_INVALID) opens the
 * generic kernel's multi-bit form: the domain becomes the same N, k and pbs_l limits with grouping_factor <= 3 dividing n,
 * without the tuned multi-bit build's restriction to pbs_l = 1, N >= 1024.  With ALLOW, a multi-bit shape that the tuned
 * multi-bit build serves (k = 1, pbs_l = 1, N in {1024, 2048}) still runs tuned and every other multi-bit shape of the
 * domain runs generic - also a tuned classical shape whose multi-bit form does not exist (k = 1, N = 512; pbs_l = 2); with
 * FORCE every launch runs generic, the tuned multi-bit sets included.  Shapes with grouping_factor <= 1 behave exactly as
 * without the bit, and without the bit every multi-bit refusal above stands.  The creation-time capacity bound is only a
 * necessary condition for a multi-bit context, tuned or generic: a group step sums 2^grouping_factor subsets' products, so
 * helm_si_load_bootstrap_key checks the key at hand - B/2 x the largest l1-norm (key words as centred 64-bit integers) over
 * the polynomials of a group, all subsets and levels, that meet in one column or one row must stay below
 * p0 p1 / 2 / 1.001 - and otherwise returns HELM_ERR_INVALID ("... capacity ...") and leaves the context as it was, usable
 * for another key.  Keys with the noise and size of a tfhe parameter set stay well below it (about 0.71 of the limit for a
 * uniformly random key at k = 1, N = 2048, pbs_logB = 21, grouping_factor = 3).
 * HELM_SI_CREATE_LARGE_N (alone or beside the bits above) admits the one shape above the generic domain: k = 1, N = 4096,
 * pbs_l >= 1, grouping_factor <= 1 - every 5-bit set (message_modulus * carry_modulus = 32).  It matters at N >= 4096 only:
 * on any smaller N the call is the same call without the bit, and without the bit every call is what it was.  With it, such
 * a shape passes every other check of helm_si_ctx_create in the same order (n, the decompositions,
 * message_modulus * carry_modulus <= N/2, and the capacity bound with the product of ITS pair of fields:
 * 2 pbs_l N 2^(pbs_logB-1) 2^63 x 1.001 < p0 p1 / 2 = 2^97.87 - one level of 22 bits is at 0.547 of it, 23 bits are refused)
 * and its bootstraps run on k_pbs64_large: one workgroup of 1024 threads per bootstrap, one per CU, in the pair 5072^4 + 1
 * and 5440^4 + 1 (helm_si_field_bits() returns 50, helm_si_kernel_class() 2).  Everything above the bootstrap kernel works
 * unchanged, many-LUT included.  Refused with a message that names the large-N domain: k > 1 at N = 4096, multi-bit at
 * N = 4096, and N = 8192 (that size has a kernel and a bit of its own: HELM_SI_CREATE_N8192, below).  helm_wop_ctx_create
 * refuses a PBS-side context of this class, and the bound-checking build refuses the class at creation.
 * HELM_SI_CREATE_PBS_KS (alone or beside any admitted combination of the bits above) chooses the other ciphertext order of a
 * tfhe shortint set (EncryptionKeyChoice::Small, the PARAM_*_PBS_KS sets): wire rows are LWE ciphertexts under the SMALL key,
 * n + 1 words, and a look-up is programmable bootstrap small->big, then keyswitch big->small.  The keys are the same keys in
 * the same layouts, and the bit changes no admission rule: the same shapes are admitted and refused with the same messages,
 * the capacity check and the kernel class chosen are those of the call without it.  What changes is the row width of
 * everything that holds wire rows (helm_si_wire_words) and the launch sequence of a look-up: ONE bootstrap launch whose jobs
 * read their input rows straight from the wire table and write big rows into the context's stage buffer, then ONE keyswitch
 * whose jobs take stage rows to table rows.  Every input row is read before any output row is written, so a call whose
 * output row is its own or another job's input row leaves what the call without the bit leaves for the same hazard (the
 * plaintexts under it; the words differ, they are ciphertexts under another key).  helm_si_apply_luts,
 * helm_si_apply_many_luts (n_out keyswitches per rotation, none for an output of -1), helm_si_eval_lut_level and
 * helm_si_set_level_many_lut follow it, lanes and the audit hook included.  Under an exchange a rank bootstraps its chunk,
 * keyswitches it into its exchange slot, rows of n + 1 words are gathered and scattered; capacity_rows counts rows whatever
 * their width, and the table is word for word the unsharded one.  helm_wop_ctx_create refuses such a PBS side by name (its
 * bit extraction, circuit bootstrap and result rows assume big rows).  The bound-checking build admits the order: nothing in
 * it depends on the row width.
 * HELM_SI_CREATE_N8192 (alone or beside any combination of the bits above) admits k = 1, N = 8192, pbs_l >= 1,
 * grouping_factor <= 1 - every 6-bit set (message_modulus * carry_modulus = 64: tfhe's MESSAGE_3_CARRY_3 and
 * MESSAGE_2_CARRY_4), the plaintext space a 6-input look-up table needs.  It matters at N = 8192 only: on any smaller N
 * the call is the same call without the bit (same status, message, class and field), and without the bit every call is
 * what it was, N = 8192 under HELM_SI_CREATE_LARGE_N alone included.  Beside HELM_SI_CREATE_LARGE_N, N selects the kernel.
 * Such a shape passes every other check of helm_si_ctx_create in the same order, the capacity bound with the product of
 * the large-N pair: 2 pbs_l N 2^(pbs_logB-1) 2^63 x 1.001 < p0 p1 / 2 = 2^97.87 - one level of 21 bits is at 0.547 of it,
 * 22 bits are refused, tfhe's 2 levels of 15 bits are at 2^92.  Its bootstraps run on k_pbs64_n8192: one workgroup of 1024
 * threads per bootstrap, one per CU, the accumulator in a row of device memory that belongs to the launching context (a
 * primary and each lane have their own; a batch wider than a round goes out in chunks of a round).  helm_si_field_bits()
 * returns 50, helm_si_kernel_class() 3, helm_si_round_capacity() the CU count.  Everything above the bootstrap kernel works
 * unchanged: keyswitch at in_dim = 8192, many-LUT, both look-up orders, lanes, audit, sharding.  Refused with a message that
 * names HELM_SI_CREATE_N8192: k > 1 at N = 8192, multi-bit at N = 8192, and N >= 16384.  helm_wop_ctx_create refuses a
 * PBS-side context of this class by name, and the bound-checking build refuses the class at creation.
 * HELM_SI_CREATE_LARGE_MULTIBIT (only together with HELM_SI_CREATE_LARGE_N and/or HELM_SI_CREATE_N8192; alone, or beside the
 * generic bits only, it is HELM_ERR_INVALID) opens the multi-bit form of the two kernels above: with bit 32 it admits k = 1,
 * N = 4096, pbs_l >= 1, grouping_factor 2 or 3 dividing n on k_pbs64_large (class 2, field bits 50); with bit 256 the same at
 * N = 8192 on k_pbs64_n8192 (class 3, round capacity = CU count); with both, N selects the kernel.  Every other check applies
 * in the same order.  The bit changes nothing (same status, message, class and field) for grouping_factor <= 1 and for any
 * N < 4096; HELM_SI_CREATE_PBS_KS beside it changes no admission rule, as beside every other bit.
 * Refused with a message that names the bit: k > 1, grouping_factor >= 4 or not dividing n, N >= 16384.  helm_wop_ctx_create
 * and the bound-checking build refuse these contexts by their class.  As for HELM_SI_CREATE_GENERIC_MULTIBIT, the
 * creation-time capacity check stays the classical one, a necessary condition only: helm_si_load_bootstrap_key applies the
 * group-sum rule above with the product of THIS pair, p0 p1 / 2 = 2^97.87, margin 1.001, and refuses a key beyond it with a
 * "capacity" message that names the large-N or the N = 8192 multi-bit kernel and gives the ratio; the context keeps the key
 * and state it had.  A uniformly random key loads when pbs_l 2^(pbs_logB + grouping_factor + 62 + log2 N) is below that:
 * one level at N = 4096 up to pbs_logB + grouping_factor = 23, at N = 8192 up to 22; two levels of 15 bits at every grouping
 * factor.  So N = 8192, one level of 21 bits, grouping factor 2 is admitted here and refused at load.
 * Unknown flag bits (4 and 8 are reserved, 128 and 512 are not assigned): HELM_ERR_INVALID. */
int helm_si_ctx_create_ex(int device_id, const helm_si_params *params, int flags, helm_si_ctx **out);
/* Which kernel runs this context's bootstraps: 0 = a tuned build, 1 = the generic kernel (k_pbs64_generic), 2 = the large-N
 * kernel (k_pbs64_large: k = 1, N = 4096 under HELM_SI_CREATE_LARGE_N, whatever generic bits stand beside it), 3 = the
 * N = 8192 kernel (k_pbs64_n8192: k = 1, N = 8192 under HELM_SI_CREATE_N8192, likewise).  Unlike
 * helm_hip_kernel_class of the boolean engine, which reports the parameter shape only (its forcing is a debug variable),
 * this reports the kernel the launches actually run on: HELM_SI_CREATE_FORCE_GENERIC is part of this API, so a forced
 * tuned shape reports 1.  A lane reports its primary's class.  Negative on error. */
int helm_si_kernel_class(const helm_si_ctx *ctx);
/* The ciphertext order of the context, numbered as helm_hip_pbs_order of the boolean engine: 1 = keyswitch, then bootstrap
 * (wire rows under the big key; every context made without HELM_SI_CREATE_PBS_KS), 0 = bootstrap, then keyswitch.  A lane
 * reports its primary's order.  Negative on error. */
int helm_si_pbs_order(const helm_si_ctx *ctx);
/* Words of a wire row: k*N + 1 in order 1, n + 1 in order 0.  The width of the rows of helm_si_wires_*, helm_si_lincomb, the
 * exchange buffers (stage_dev, gather_dev) and the audit records.  A lane reports its primary's width.  Negative on error. */
int64_t helm_si_wire_words(const helm_si_ctx *ctx);
int helm_si_ctx_destroy(helm_si_ctx *ctx);
/* A lane: a second context on the same device that shares `primary`'s keys and may work on its wire tables, with
 * its own stream and scratch - independent parts of a circuit can then be evaluated concurrently (one host thread
 * per lane; the GPU overlaps their launches).  The reference's unit of parallelism is the level
 * (src/circuit.rs:1057, 1321: par_iter over the gates of a level); lanes add parallelism ACROSS levels for
 * sub-circuits that share no wire.  Fork after the keys are loaded; destroy every lane before its primary.
 * Rows written through one lane must not be touched through another until both have been synchronised.
 * A lane holds its primary's key state - keys, transform tables, CRT pair - not a copy of it: a key loaded into the primary
 * later is the key every lane launches with from then on (helm_si_field_bits of a lane follows it), and keys are loaded
 * into the primary only (below). */
int helm_si_ctx_fork(helm_si_ctx *primary, helm_si_ctx **lane_out);
int helm_si_get_params(const helm_si_ctx *ctx, helm_si_params *out);
/* The CRT pair of prime fields the bootstrap kernels of this context compute in, as its size class: 49 = 5072^4 + 1 and
 * 5096^4 + 1 (every parameter set up to N = 2048), 50 = 5072^4 + 1 and 5440^4 + 1 (the large-N kernel: N = 4096, where
 * 5096^4 + 1 has no 2N-th root of unity; fixed for the context's life), 46 = 2736^4 + 1 and 2872^4 + 1 - k > 1 contexts (k_pbs64k: the set reference
 * src/bin/helm.rs:301 installs for LUT mode) whose LOADED key keeps the exact products of a blind-rotation step below
 * p p' / 2 = 2^90.6: helm_si_load_bootstrap_key computes B/2 x the largest l1-norm of a key column for the key at hand (an
 * exact guarantee for that key and every input; a generated key fits, the worst case of the set does not and keeps 49), so
 * the value may change when a key is loaded (HELM_SI_FIELD=49 in the environment keeps the 49-bit pair).  Results do not
 * depend on it (exact integer arithmetic either way); reported because the operation count of the kernel does: the smaller
 * primes leave 2^53 / p >= 128 of headroom, so both leading stages of a forward transform on 17-bit digits are plain
 * multiplications and most recentrings go.  Negative on error. */
int helm_si_field_bits(const helm_si_ctx *ctx);
int helm_si_set_stream(helm_si_ctx *ctx, void *hip_stream);
int helm_si_sync(helm_si_ctx *ctx);
/* Dispatch priority of the context's OWN stream (no effect after helm_si_set_stream): high != 0 = the device's highest
 * stream priority, 0 = its lowest.  When two lanes have launches ready at the same time the workgroups of the
 * high-priority one are placed first - the host library gives it to the lane with the longest chain of bootstrap rounds.
 * Synchronises the stream it replaces. */
int helm_si_set_priority(helm_si_ctx *ctx, int high);
/* Keys are loaded into a primary context; a lane refuses them with HELM_ERR_INVALID and touches nothing (its keys are its
 * primary's).  A key may be loaded again, into a primary that has lanes too: the load first synchronises the primary's
 * stream and the stream of every lane forked from it, then rewrites the shared tables and key buffers, and every lane
 * sees the new key.  The caller does not load while another thread drives one of the lanes. */
int helm_si_load_bootstrap_key(helm_si_ctx *ctx, const uint64_t *bsk_std, size_t n_words);
int helm_si_load_keyswitch_key(helm_si_ctx *ctx, const uint64_t *ksk, size_t n_words);

/* Device-resident ciphertext table (replaces HashMap<String, Arc<RwLock<CtxtShortInt>>>,
 * circuit.rs:1046-1049).  Rows of helm_si_wire_words() words: k*N+1, or n+1 under HELM_SI_CREATE_PBS_KS. */
int helm_si_wires_alloc(helm_si_ctx *ctx, int64_t n_rows, helm_si_wires **out);
int helm_si_wires_free(helm_si_ctx *ctx, helm_si_wires *w);
int helm_si_wires_upload(helm_si_ctx *ctx, helm_si_wires *w, const int32_t *idx, const uint64_t *lwe_host,
                         int64_t count);
int helm_si_wires_download(helm_si_ctx *ctx, helm_si_wires *w, const int32_t *idx, uint64_t *lwe_host,
                           int64_t count);
/* Row copy between two tables of the same context (Ciphertext::clone, circuit.rs:1046-1049). */
int helm_si_wires_copy(helm_si_ctx *ctx, helm_si_wires *src, const int32_t *src_idx, helm_si_wires *dst,
                       const int32_t *dst_idx, int64_t count);
/* ServerKey::create_trivial(value) (circuit.rs:978): zero mask, body = value * delta. */
int helm_si_wires_set_trivial(helm_si_ctx *ctx, helm_si_wires *w, const int32_t *idx, const uint64_t *value,
                              int64_t count);

/* out[g] = sum_{t<terms} coef[g*terms+t] * row in_idx[g*terms+t]  +  const_add[g] * delta
 * (in_idx = -1: term skipped).  Replaces unchecked add / sub / scalar_mul /
 * scalar_left_shift / neg / scalar_add of tfhe::shortint (gates.rs:769,776-778). */
int helm_si_lincomb(helm_si_ctx *ctx, helm_si_wires *w, const int32_t *in_idx, const int64_t *coef,
                    const int64_t *const_add, const int32_t *out_idx, int32_t terms, int64_t count);

/* Look-up tables as test polynomials (n_luts rows of N words), see layout above.
 * helm_si_make_lut() is ServerKey::generate_lookup_table(f) with f given as its value
 * table over [0, message_modulus*carry_modulus). */
int helm_si_make_lut(const helm_si_ctx *ctx, const uint64_t *f_values, uint64_t *test_poly_out);
/* out[g] = apply_lookup_table(row in_idx[g], luts[lut_idx[g]])  (gates.rs:783): keyswitch
 * then programmable bootstrap, `count` ciphertexts in one batched dispatch. */
int helm_si_apply_luts(helm_si_ctx *ctx, helm_si_wires *w, const int32_t *in_idx, const int32_t *lut_idx,
                       const int32_t *out_idx, int64_t count, const uint64_t *luts, int64_t n_luts);

/* Many-LUT bootstrap: several functions of one input from ONE blind rotation (later tfhe releases:
 * ServerKey::generate_many_lookup_table / apply_many_lookup_table).  With t = message_modulus * carry_modulus, box = N / t,
 * n_funcs >= 1 and M = the smallest power of two >= n_funcs (M <= t), the test polynomial holds function i in chunk i of
 * N / M coefficients: before the rotation, coefficient (i * (t / M) + v) * box + j is f_i(v) * delta for i < n_funcs,
 * v < t / M, j < box; chunks i >= n_funcs are zero; then, as helm_si_make_lut, the first box / 2 coefficients are negated
 * and the polynomial is rotated left by box / 2.  f_values is [n_funcs][t / M].  n_funcs = 1 gives helm_si_make_lut's
 * polynomial word for word.  n_funcs < 1, M > t or a null pointer: HELM_ERR_INVALID.
 * INPUT BOUND: such a table answers correctly only for an input v < t / M (as a ciphertext's degree in tfhe: a 2+2-bit
 * block after one addition holds at most 6 < 8 = t / 2, so message v % 4 and carry v / 4 are two functions of one
 * rotation).  The bound is the caller's responsibility; nothing checks it on the device. */
int helm_si_make_many_lut(const helm_si_ctx *ctx, const uint64_t *f_values, int32_t n_funcs, uint64_t *test_poly_out);
/* For each g < count: keyswitch row in_idx[g], ONE blind rotation with table lut_idx[g], then n_out sample extracts: output
 * x < n_out is the extract at coefficient h = x * N / M of the rotated accumulator (A_0 .. A_{k-1}, B), M = the power of two
 * >= n_out - mask word r * N + u is A_r[h - u] for u <= h and -A_r[N + h - u] for u > h, the body is B[h] (h = 0: what
 * helm_si_apply_luts extracts) - and is written to row out_idx[g * n_out + x]; -1 there skips that output.  As
 * helm_si_apply_luts: every keyswitch finishes before any output row is written (an output may be an input row), row
 * indices are range-checked, lanes work alike, and n_out = 1 gives the rows of helm_si_apply_luts.  Two outputs of one call
 * naming the same row, n_out < 1 or M > t: HELM_ERR_INVALID.  helm_si_get_timing counts blind rotations: pbs_count rises by
 * count, not by count * n_out.  Under an exchange (helm_si_set_exchange*) a batch of at least min_batch
 * ciphertexts is sharded as helm_si_apply_luts shards: `world` contiguous chunks of ciphertexts, this rank keyswitches and
 * rotates its chunk only, its chunk * n_out extracted rows go into its exchange slot (row g * n_out + x of the chunk), the
 * collective runs, and the gathered rows are scattered to out_idx without the -1 outputs.  capacity_rows counts rows: a round
 * holds at most capacity_rows / n_out ciphertexts per rank (larger batches go in several rounds), and n_out > capacity_rows
 * is HELM_ERR_INVALID.  This rank keyswitches its share of every round before the first round is scattered, so the table is
 * word for word what the unsharded call leaves - also where an output row of an early ciphertext is the input row of a later
 * one.  helm_si_exchange_stats counts these rounds and rows; pbs_count rises by this rank's ciphertexts.  The host library's
 * operators use this call on request (helm_host_si_circuit_set_many_lut, helm_host_radix_level_ex in helm_host.h). */
int helm_si_apply_many_luts(helm_si_ctx *ctx, helm_si_wires *w, const int32_t *in_idx, const int32_t *lut_idx,
                            const int32_t *out_idx, int32_t n_out, int64_t count, const uint64_t *luts, int64_t n_luts);

/* One netlist level of LUT gates = gates::lut() per gate (gates.rs:754-785):
 *   arity 1  : table all zero -> copy, else -> negation (smart_neg)
 *   arity 2  : bivariate f(x,y) = table[(x&1)*2 + (y&1)]
 *   arity >=3: pack sum in_i << (arity-1-i) (first input = MSB, gates.rs:159-167),
 *              f(x) = table[x] & 1
 * arity 0 with table 0: DFF / copy of in_idx[g*max_in] (circuit.rs:1063-1069).
 * table[g] holds the truth table as bits (bit i = entry i), in_idx is [count][max_in]. */
int helm_si_eval_lut_level(helm_si_ctx *ctx, helm_si_wires *w, const int32_t *arity, const int32_t *in_idx,
                           int32_t max_in, const uint64_t *table, const int32_t *out_idx, int64_t count);
/* LUT levels that share rotations (default 0: off; a lane forked afterwards inherits the setting).  With on != 0,
 * helm_si_eval_lut_level groups the bootstrapped gates of a level that have the same arity and the identical input rows in the
 * same order: they pack the same index, which is below 2^arity, so up to M = t >> arity of them (the largest M with
 * 2^arity <= t / M; t = message_modulus * carry_modulus) are the functions of one many-LUT table and cost ONE blind rotation -
 * M = 2 for arity 3 and M <= 4 for arity 2 at t = 16, M = 2 for arity 2 at t = 8, no grouping at t = 4 or where
 * 2^arity = t.  A full adder (0x96 and 0xE8 on the same three inputs) is one rotation instead of two.  The index of a group is
 * packed once, into its first gate's output row; the level's groups are the jobs of ONE helm_si_apply_many_luts dispatch
 * (sharded and audited as that call: kind 2 records) with n_out = M_d, the largest group's power of two: gate i of a group
 * of n is output i * M_d / M_n (M_n = the power of two >= n), the other outputs are skipped.  A gate without a partner rides
 * in the same dispatch with helm_si_make_lut's table and output 0 only: its row is word for word what the setting off
 * gives.  A level without any group is evaluated exactly as with the setting off (helm_si_apply_luts).  Gates of arity 0 / 1,
 * flip-flops and every refusal of helm_si_eval_lut_level are unchanged.  Test polynomials are built once per distinct tuple
 * of functions per level. */
int helm_si_set_level_many_lut(helm_si_ctx *ctx, int on);

/* Multi-GPU (one process per GPU, keys and wire tables replicated): after this call every
 * bootstrap batch of at least `min_batch` ciphertexts - helm_si_apply_luts() and everything
 * built on it: helm_si_eval_lut_level(), the radix operators of the host library - is split
 * into `world` contiguous chunks.  This rank keyswitches and bootstraps chunk `rank` into
 * `stage_dev` (rows of helm_si_wire_words() words), calls fn(user, rows_per_rank), which must all-gather
 * rows_per_rank rows of stage_dev from every rank into gather_dev in rank order ON THE
 * CONTEXT'S STREAM (ncclAllGather over RCCL/xGMI; helm_si_set_stream) and return 0, and then
 * scatters the gathered rows into the table.  Every rank must issue the same calls in the same
 * order; the ciphertexts are identical to a single-GPU evaluation.  stage_dev holds
 * capacity_rows rows, gather_dev capacity_rows * world (larger batches go in several rounds).
 * world < 1, or world = 1 without a callback, switches sharding off (world = 1 WITH a callback keeps
 * every batch on the stage -> collective -> scatter path: the single-GPU test of it).  The reference
 * has no multi-GPU path; its unit of parallelism is the level (src/circuit.rs:1057 par_iter_mut over
 * the gates of a level). */
typedef int (*helm_si_exchange_fn)(void *user, int64_t rows_per_rank);
int helm_si_set_exchange(helm_si_ctx *ctx, int32_t rank, int32_t world, int64_t min_batch, void *stage_dev,
                         void *gather_dev, int64_t capacity_rows, helm_si_exchange_fn fn, void *user);
/* The same with the collective INSIDE the library: the all-gather is ncclAllGather through `comm`
 * (include/helm_comm.h; rank and world are the communicator's) on the context's stream, into a gather
 * buffer of capacity_rows * world rows the context allocates; this rank's chunk is bootstrapped straight
 * into its slot of that buffer (all-gather in place).  No callback, no host framework - what a Rust host calls.
 * comm = NULL switches sharding off.  The communicator must outlive the setting. */
struct helm_comm;
int helm_si_set_exchange_comm(helm_si_ctx *ctx, struct helm_comm *comm, int64_t min_batch, int64_t capacity_rows);
/* batches sharded so far and rows moved through gather_dev (per rank) */
int helm_si_exchange_stats(const helm_si_ctx *ctx, int64_t *batches, int64_t *rows);
/* the `world` of helm_si_set_exchange (1: sharding off).  A lane does not inherit the exchange of its primary: callers
 * that shard keep to the primary context (the host library's ArithCircuit does not fork its default lane then). */
int helm_si_exchange_world(const helm_si_ctx *ctx);

/* Audit (tracing): while a callback is set, every helm_si_lincomb(), helm_si_apply_luts() and helm_si_apply_many_luts() call - and with them everything
 * built on the two: helm_si_eval_lut_level(), the LUT-mode and arithmetic-mode evaluators of the host library - copies its
 * operand rows (read BEFORE the call runs: a batch may work in place) and its result rows to the host and hands them to
 * `fn` together with the call's arguments; a non-zero return fails the call.  How tests/test_gpu_audit.py checks whole
 * evaluations at the full parameter sets against the CPU oracle, operation by operation (each batch's outputs == the
 * oracle's on the GPU's own inputs, hence every wire).  Slow by construction (two synchronous copies per call); lanes
 * forked AFTER this call inherit it.  fn = NULL switches it off.  The rows handed over are wire rows of the context's width,
 * helm_si_wire_words() words each: k*N+1 in order 1, n+1 under HELM_SI_CREATE_PBS_KS. */
typedef struct {
    int32_t kind;             /* 0 = helm_si_apply_luts, 1 = helm_si_lincomb, 2 = helm_si_apply_many_luts (fields as kind 0, but
                               * terms = n_out and out_rows = count * n_out rows, output x of ciphertext g at row g * n_out + x,
                               * a skipped output: zeros) */
    int32_t terms;            /* lincomb: operands per output; apply_many_luts: n_out */
    int64_t count, n_luts;
    const uint64_t *in_rows;  /* apply_luts: count wire rows; lincomb: count * terms (a skipped operand: zeros) */
    const uint64_t *out_rows; /* count rows */
    const int32_t *lut_idx;   /* apply_luts */
    const uint64_t *luts;     /* apply_luts: n_luts test polynomials of N words */
    const int32_t *in_idx;    /* lincomb: the call's own arrays */
    const int64_t *coef, *const_add;
} helm_si_audit_record;
typedef int (*helm_si_audit_fn)(void *user, const helm_si_audit_record *rec);
int helm_si_set_audit(helm_si_ctx *ctx, helm_si_audit_fn fn, void *user);

/* Debug build only (-DHELM_CHECK_BOUNDS: csrc/libhelm_hip_check.so, loaded through HELM_HIP_LIB): the kernels of the 64-bit
 * engine (and of the WoP-PBS path, which shares its translation unit) count every violation of the contracts of the lazy
 * modular arithmetic, slots as in helm_hip_bound_violations (include/helm_hip.h).  The counters are per engine: the boolean
 * engine's are read through its own entry point.  The regular build returns HELM_ERR_STATE. */
int helm_si_bound_violations(helm_si_ctx *ctx, uint32_t counts[8], int reset);

/* Programmable bootstraps the device holds at once under this parameter set: CUs x workgroups of the set's bootstrap kernel
 * per CU (1 at N = 2048, 2 for k_pbs64k; on the generic kernel, its resident workgroups per CU at the context's LDS size; 1 on the large-N kernel).  A batch of at most this many ciphertexts takes one bootstrap's time whatever its
 * size; the host library merges the look-up rounds of concurrent operators into launches of at most this size. */
int64_t helm_si_round_capacity(helm_si_ctx *ctx);

/* Primitive forms on host buffers (tests).  small: count x (n+1); big: count x (k*N+1).  They work on host buffers of these
 * two widths whatever the context's order: HELM_SI_CREATE_PBS_KS changes nothing about them. */
int helm_si_keyswitch_batch(helm_si_ctx *ctx, const uint64_t *in_big, uint64_t *out_small, int64_t count);
int helm_si_pbs_batch(helm_si_ctx *ctx, const uint64_t *in_small, const uint64_t *luts, int64_t n_luts,
                      const int32_t *lut_idx, uint64_t *out_big, int64_t count);
/* The many-LUT primitive (helm_si_apply_many_luts without the keyswitch): out_big is count * n_out rows, output x of
 * ciphertext g at row g * n_out + x. */
int helm_si_pbs_many_batch(helm_si_ctx *ctx, const uint64_t *in_small, const uint64_t *luts, int64_t n_luts,
                           const int32_t *lut_idx, int32_t n_out, uint64_t *out_big, int64_t count);

typedef struct {
    double pbs_ms, ks_ms, linear_ms;
    int64_t pbs_launches, pbs_count, ks_launches, ks_count;
} helm_si_timing;
int helm_si_timing_enable(helm_si_ctx *ctx, int enable);
int helm_si_get_timing(helm_si_ctx *ctx, helm_si_timing *out, int reset);

#ifdef __cplusplus
}
#endif
#endif /* HELM_SHORTINT_H */
