// many_lut_rule.h - which gates of a LUT level may share one blind rotation (helm_si_set_level_many_lut).
//
// One definition, used by the engine (helm_shortint.hip: helm_si_eval_lut_level groups by it) and by the host library
// (LutCircuit counts the rotations of a cycle by it), so that the count a host reports is the count the engine runs.
#ifndef HELM_MANY_LUT_RULE_H
#define HELM_MANY_LUT_RULE_H

namespace helm_many_lut {

// How many gates of `arity` inputs on the same input tuple may share a rotation at plaintext space t = message x carry:
// the largest M with 2^arity <= t / M - a many-LUT table of M chunks answers for an index below t / M, and the packed index
// of such a gate is below 2^arity.  1 = no sharing: arity below 2 (no bootstrap), or an index that needs the whole space.
inline int group_max(int arity, int t) { return arity >= 2 && arity < 31 && (1 << arity) <= t ? t >> arity : 1; }

} // namespace helm_many_lut
#endif
