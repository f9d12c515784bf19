// wide_share_rule.h - which wide LUT gates of a level form one group of helm_wop_eval_many_luts (include/helm_wopbs.h).
//
// Every stage of a wide gate but its table look-up and the way back depends on the gate's input rows alone, so gates that
// read the same rows IN THE SAME ORDER can share those stages: the eight output bits of an S-box, the bits of a small ROM.
// Gates whose inputs are a permutation of each other are NOT grouped: the extracted bits would index the table in another
// order, and rewriting the table is out of scope.
//
// One definition, used by LutCircuit (shortint_circuit.cpp) and exported through libhelm_host.so (helm_host_wide_lut_groups,
// helm_host_wide_lut_group_cap) so that the CPU tests see the rule the host applies.
#ifndef HELM_WIDE_SHARE_RULE_H
#define HELM_WIDE_SHARE_RULE_H

#include <cstdint>
#include <map>
#include <vector>

namespace helm_wide_share {

// the most tables one group takes: what one pass of a chunk holds (helm_wop_eval_many_luts: max(1, 16384 / bits))
inline int64_t group_cap(int bits) { return bits < 1 ? 0 : (16384 / bits > 1 ? 16384 / bits : 1); }

// Gates 0 .. count-1 with input rows in_idx[count][n_inputs].  group_of[g] = the group of gate g; groups are numbered by their
// first gate, a group's gates keep the order of the call, and a group that holds `cap` gates is closed - the next gate on
// the same tuple opens a new one.  Returns the number of groups.
inline int64_t group_gates(const int32_t *in_idx, int64_t count, int n_inputs, int64_t cap, int64_t *group_of)
{
    std::map<std::vector<int32_t>, std::pair<int64_t, int64_t>> open; // tuple -> (group, members)
    int64_t groups = 0;
    for (int64_t g = 0; g < count; g++) {
        std::vector<int32_t> key(in_idx + g * n_inputs, in_idx + (g + 1) * n_inputs);
        auto it = open.find(key);
        if (it == open.end() || it->second.second >= cap) {
            open[key] = {groups, 1};
            group_of[g] = groups++;
        } else {
            it->second.second++;
            group_of[g] = it->second.first;
        }
    }
    return groups;
}

} // namespace helm_wide_share
#endif
