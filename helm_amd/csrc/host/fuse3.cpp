// fuse3.cpp — the opt-in three-input fusion pass of gates mode (include/helm_host.h: helm_host_fuse3).
//
// Under the boolean encoding (true = +1/8, false = -1/8) the sum of three ciphertexts has the sign of their majority and
// twice the sum carries their parity, so MAJ3 / XOR3 / XNOR3 are ONE bootstrap each (HELM_GATE_MAJ3 / XOR3 / XNOR3,
// pbs_frame.h: gate_lincomb).  A full adder written with two-input gates is five bootstraps on two levels per bit; as
// xor3 + maj it is two bootstraps on one level per bit.  The pass rewrites exactly two patterns, to a fixed point, visiting
// the gates in netlist order (so its output is deterministic):
//
//   R1 (parity)  G = xor|xnor(u, v), two inputs, where u or v - the deeper of the two (in bootstraps) is tried first, u on a
//                tie - is driven by I = xor|xnor(a, b), two inputs: G becomes xor3(a, b, other) - xnor3 when an odd number
//                of G and I are xnor - and I is deleted.  Not when `other` is a or b, or a is b: the three operands of a
//                fused gate are three wires, so that its operand is a sum of three DIFFERENT ciphertexts (a repeated
//                one would enter with weight 2 and leave the noise budget stated for the gate).
//   R2 (carry)   G = or(p, q) with p = and(a, b) and q = and(x, c) or and(c, x), in either operand order of the or, where
//                x = xor(a, b) or or(a, b) (operands in either order): G becomes maj(a, b, c); p and q are deleted, x stays
//                (R1 may pick it up on the next sweep, once its fan-out has dropped).  a, b, c are three wires, as in R1.
//                ab + c(a ^ b) = ab + c(a | b) = majority(a, b, c).
//
// A gate is deleted only when exactly one gate input reads its output (a dff or mux counts as a reader like any other)
// and that output is no module output.  The surviving gate keeps its name, its output wire and its line's indentation;
// every line the pass does not rewrite is passed through as it is.  lut, arithmetic gates, mux, dff, constants and
// n-ary forms are never touched.  Both rules only remove gates and never deepen one, so neither the bootstrap count nor
// the number of bootstrapped levels grows; on the fixed point no pattern is left, so a second run changes nothing.
#include "helm_host.hpp"

#include <set>
#include <sstream>
#include <unordered_map>
#include <unordered_set>

namespace helm {

namespace {

struct Item {
    std::string line;   // the line as it came (without its newline)
    bool is_gate = false;
    bool alive = true;  // false: deleted by a rule
    bool rewritten = false;
    bool binary_form = false; // `<kw> NAME(in0, in1, out);` - four tokens
    GateType type = GateType::Buf;
    std::string name, out;
    std::vector<std::string> ins;
};

std::string trim(const std::string &s)
{
    size_t a = 0, b = s.size();
    while (a < b && isspace((unsigned char)s[a])) a++;
    while (b > a && isspace((unsigned char)s[b - 1])) b--;
    return s.substr(a, b - a);
}

// the parser's tokens of a line (netlist.cpp: split at ',' and ' ', empty pieces dropped)
std::vector<std::string> tokens_of(const std::string &line)
{
    std::vector<std::string> out;
    std::string cur;
    for (char ch : line) {
        if (ch == ',' || ch == ' ') {
            if (!cur.empty()) out.push_back(cur);
            cur.clear();
        } else
            cur.push_back(ch);
    }
    if (!cur.empty()) out.push_back(cur);
    return out;
}

bool starts_with(const std::string &s, const char *p) { return s.rfind(p, 0) == 0; }

int bootstraps_of(GateType t)
{
    switch (t) {
    case GateType::And: case GateType::Nand: case GateType::Or: case GateType::Nor: case GateType::Xor: case GateType::Xnor:
    case GateType::Maj3: case GateType::Xor3: case GateType::Xnor3: case GateType::Lut: return 1;
    case GateType::Mux: return 2;
    default: return 0;
    }
}

bool is_parity(GateType t) { return t == GateType::Xor || t == GateType::Xnor; }

const char *keyword_of(GateType t)
{
    return t == GateType::Maj3 ? "maj" : t == GateType::Xor3 ? "xor3" : "xnor3";
}

// {bootstraps, bootstrapped levels} of a netlist text.  Bootstrapped levels = the longest chain of bootstrapped gates from
// an input or a flip-flop output to any wire: what one evaluation waits for in a row.  Gates without a bootstrap (not,
// buf, constants) add no level.  Walked in the order of the circuit's own levelling (ascending level_map).
void count(const std::string &text, int64_t &bootstraps, int64_t &levels)
{
    verilog_parser::Netlist nl = verilog_parser::read_verilog_text(text, false);
    Circuit c(nl.gates, nl.inputs, nl.outputs, nl.dff_outputs);
    c.sort_circuit();
    c.compute_levels();
    bootstraps = levels = 0;
    std::unordered_map<std::string, int64_t> chain; // wire -> bootstraps in a row behind it (absent: 0)
    for (auto &kv : c.level_map())
        for (auto &g : kv.second) {
            if (g.get_gate_type() == GateType::Dff) continue; // its output is an input of the cycle
            const int w = bootstraps_of(g.get_gate_type());
            bootstraps += w;
            int64_t deepest = 0;
            for (auto &in : g.get_input_wires()) {
                auto it = chain.find(in);
                if (it != chain.end() && it->second > deepest) deepest = it->second;
            }
            const int64_t here = deepest + (w > 0 ? 1 : 0);
            chain[g.get_output_wire()] = here;
            if (here > levels) levels = here;
        }
}

} // namespace

std::string fuse3(const std::string &text, int64_t stats[4])
{
    count(text, stats[0], stats[2]); // (also refuses what the parser refuses)

    // the lines; gate lines parsed with the parser's own parse_gate, a second gate of a name passed through (the parser
    // drops it: GateSet keeps the first)
    std::vector<Item> items;
    std::set<std::string> names;
    {
        std::istringstream in(text);
        std::string raw;
        while (std::getline(in, raw)) {
            Item it;
            it.line = raw;
            const std::string line = trim(raw);
            const std::vector<std::string> tok = tokens_of(line);
            if (!line.empty() && !tok.empty() && !starts_with(line, "module") && !starts_with(line, "endmodule") &&
                !starts_with(line, "//") && tok[0] != "input" && tok[0] != "output" && tok[0] != "wire") {
                Gate g = verilog_parser::parse_gate(tok);
                if (names.insert(g.get_gate_name()).second) {
                    it.is_gate = true;
                    it.type = g.get_gate_type();
                    it.name = g.get_gate_name();
                    it.out = g.get_output_wire();
                    it.ins = g.get_input_wires();
                    it.binary_form = tok.size() == 4 && it.ins.size() == 2;
                }
            }
            items.push_back(std::move(it));
        }
    }
    const verilog_parser::Netlist nl = verilog_parser::read_verilog_text(text, false);
    const std::unordered_set<std::string> module_out(nl.outputs.begin(), nl.outputs.end());

    std::unordered_map<std::string, int> readers;  // wire -> gate inputs that read it
    std::unordered_map<std::string, long> driver;  // wire -> the gate that drives it (-1: more than one does)
    for (size_t i = 0; i < items.size(); i++) {
        if (!items[i].is_gate) continue;
        for (auto &w : items[i].ins) readers[w]++;
        auto ins = driver.emplace(items[i].out, (long)i);
        if (!ins.second) ins.first->second = -1;
    }
    auto driven_by = [&](const std::string &w) -> long {
        auto it = driver.find(w);
        return it == driver.end() ? -1 : it->second;
    };
    auto deletable = [&](const Item &g) { return readers[g.out] == 1 && !module_out.count(g.out); };
    auto remove = [&](Item &g) {
        g.alive = false;
        for (auto &w : g.ins) readers[w]--;
        driver.erase(g.out);
    };
    auto become = [&](Item &g, GateType t, std::vector<std::string> ins) {
        for (auto &w : g.ins) readers[w]--;
        g.type = t;
        g.ins = std::move(ins);
        for (auto &w : g.ins) readers[w]++;
        g.rewritten = true;
        g.binary_form = false;
    };

    // Depth of every wire in bootstraps (inputs, flip-flop outputs and constants 0; a bootstrapped gate's output one more
    // than its deepest input, a not / buf as deep as its input), taken
    // at the start of a sweep: when both operands of a parity gate could be absorbed, R1 absorbs the DEEPER one - that is
    // the one whose removal can shorten the path.  (A sweep only ever makes wires shallower; a stale depth is a weaker
    // choice, never a wrong one.)
    std::unordered_map<std::string, int64_t> depth;
    auto compute_depths = [&]() {
        depth.clear();
        std::vector<std::pair<long, size_t>> stack; // (gate, next input)
        std::unordered_set<long> open;
        for (size_t root = 0; root < items.size(); root++) {
            if (!items[root].is_gate || !items[root].alive || depth.count(items[root].out)) continue;
            stack.emplace_back((long)root, 0);
            open.insert((long)root);
            while (!stack.empty()) {
                const long gi = stack.back().first;
                const Item &g = items[(size_t)gi];
                const bool source = g.type == GateType::Dff || g.type == GateType::ConstOne || g.type == GateType::ConstZero;
                if (!source && stack.back().second < g.ins.size()) {
                    const long d = driven_by(g.ins[stack.back().second++]);
                    if (d >= 0 && items[(size_t)d].alive && !depth.count(items[(size_t)d].out) && open.insert(d).second)
                        stack.emplace_back(d, 0);
                    continue;
                }
                int64_t deepest = 0;
                if (!source)
                    for (auto &w : g.ins) {
                        auto it = depth.find(w);
                        if (it != depth.end() && it->second > deepest) deepest = it->second;
                    }
                depth[g.out] = source ? 0 : deepest + (bootstraps_of(g.type) > 0 ? 1 : 0);
                open.erase(gi);
                stack.pop_back();
            }
        }
    };
    auto depth_of = [&](const std::string &w) -> int64_t {
        auto it = depth.find(w);
        return it == depth.end() ? 0 : it->second;
    };

    auto rule_parity = [&](Item &g) {
        if (!is_parity(g.type) || !g.binary_form) return false;
        const int first = depth_of(g.ins[1]) > depth_of(g.ins[0]) ? 1 : 0;
        for (int side : {first, 1 - first}) {
            const long d = driven_by(g.ins[(size_t)side]);
            if (d < 0 || &items[(size_t)d] == &g) continue;
            Item &inner = items[(size_t)d];
            if (!inner.alive || !is_parity(inner.type) || !inner.binary_form || !deletable(inner)) continue;
            const std::string &other = g.ins[(size_t)(1 - side)];
            if (inner.ins[0] == inner.ins[1] || other == inner.ins[0] || other == inner.ins[1]) continue; // three wires
            const bool odd = (g.type == GateType::Xnor) != (inner.type == GateType::Xnor);
            std::vector<std::string> ins = {inner.ins[0], inner.ins[1], g.ins[(size_t)(1 - side)]};
            become(g, odd ? GateType::Xnor3 : GateType::Xor3, std::move(ins));
            remove(inner);
            return true;
        }
        return false;
    };
    auto rule_carry = [&](Item &g) {
        if (g.type != GateType::Or || !g.binary_form || g.ins[0] == g.ins[1]) return false;
        for (int side = 0; side < 2; side++) {
            const long dp = driven_by(g.ins[(size_t)side]), dq = driven_by(g.ins[(size_t)(1 - side)]);
            if (dp < 0 || dq < 0 || dp == dq) continue;
            Item &p = items[(size_t)dp], &q = items[(size_t)dq];
            if (&p == &g || &q == &g) continue;
            if (!p.alive || !q.alive || p.type != GateType::And || q.type != GateType::And || !p.binary_form ||
                !q.binary_form || !deletable(p) || !deletable(q))
                continue;
            const std::string &a = p.ins[0], &b = p.ins[1];
            for (int xs = 0; xs < 2; xs++) { // q = and(x, c) or and(c, x)
                const long dx = driven_by(q.ins[(size_t)xs]);
                if (dx < 0) continue;
                const Item &x = items[(size_t)dx];
                if (!x.alive || !x.binary_form || (x.type != GateType::Xor && x.type != GateType::Or)) continue;
                if (!((x.ins[0] == a && x.ins[1] == b) || (x.ins[0] == b && x.ins[1] == a))) continue;
                const std::string &c = q.ins[(size_t)(1 - xs)];
                if (a == b || c == a || c == b) continue; // three wires, as in R1
                std::vector<std::string> ins = {a, b, c};
                become(g, GateType::Maj3, std::move(ins));
                remove(p);
                remove(q);
                return true;
            }
        }
        return false;
    };

    for (bool changed = true; changed;) {
        changed = false;
        compute_depths();
        for (auto &g : items)
            if (g.is_gate && g.alive && (rule_parity(g) || rule_carry(g))) changed = true;
    }

    std::string out;
    for (auto &it : items) {
        if (!it.alive) continue;
        if (it.rewritten) {
            size_t indent = 0;
            while (indent < it.line.size() && isspace((unsigned char)it.line[indent])) indent++;
            out += it.line.substr(0, indent) + keyword_of(it.type) + " " + it.name + "(" + it.ins[0] + ", " + it.ins[1] +
                   ", " + it.ins[2] + ", " + it.out + ");";
        } else
            out += it.line;
        out += '\n';
    }
    if (!text.empty() && text.back() != '\n' && !out.empty()) out.pop_back(); // no newline at the end: none added
    count(out, stats[1], stats[3]);
    return out;
}

} // namespace helm
