// Switches.cpp -- parsing and introspection of the run-time switch table (see Switches.hpp): the only translation
// unit under core/ that reads the environment.
#include "Switches.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "types.hpp"

namespace emf {

namespace {

struct Row {
    const char* field;
    const char* name;
    SwitchKind kind;
    SwitchRule rule;
    long long dflt;
    bool path;
    const char* doc;
};
const Row kRows[] = {
#define X(field, type, name, kind, rule, dflt, path, doc) {#field, name, SwitchKind::kind, SwitchRule::rule, dflt, path, doc},
    EMF_SWITCH_TABLE(X)
#undef X
};

#ifdef EMF_DEBUG_SWITCHES
constexpr bool kReadsDemoted = true;
#else
constexpr bool kReadsDemoted = false;
#endif

// A demoted switch is set in the environment of a product build: one line on stderr per variable and process, then
// ignored (a script that still sets it A/Bs two identical configurations: say so, once).
void demotedSwitchSet(const char* name) {
    if (!std::getenv(name)) return;
    static std::mutex m;
    static std::vector<std::string> warned;
    std::lock_guard<std::mutex> lock(m);
    for (const auto& w : warned)
        if (w == name) return;
    warned.emplace_back(name);
    std::fprintf(stderr, "emfusion_amd: %s is set, but this build ignores it (a switch whose A/B is on record as lost; "
                         "`make -C emfusion_amd/csrc dbg` builds libemf_fusion_dbg.so, which reads it)\n", name);
}

// one parser per rule; `v` is the variable's text, never NULL
long long parse(const Row& r, const char* v) {
    switch (r.rule) {
    case SwitchRule::OffOnZero: return v[0] != '0';
    case SwitchRule::OnOnOne: return v[0] == '1';
    case SwitchRule::Present: return 1;
    case SwitchRule::Int: return std::atoi(v);
    case SwitchRule::IntMin1: return std::max(1, std::atoi(v));
    case SwitchRule::Lanes: {
        const int lanes = std::atoi(v);
        if (lanes != 1 && lanes != 2 && lanes != 4)  // refused, not silently marched with one lane
            throw HipError(std::string("EMFusion: ") + r.name + "=" + v + " (1, 2 or 4 lanes per background ray)", EMF_E_ARG);
        return lanes;
    }
    case SwitchRule::Flags012: return v[0] == '2' ? 2 : (v[0] == '1' ? 1 : 0);
    case SwitchRule::Priority:
        if (!v[0]) return r.dflt;
        if (v[0] == 'h' || v[0] == '+' || v[0] == '1') return 1;
        if (v[0] == 'l' || v[0] == '-') return -1;
        return 0;
    case SwitchRule::MiB: return static_cast<long long>(std::strtoull(v, nullptr, 10));
    }
    return r.dflt;
}

long long valueOf(const Row& r) {
    if (r.kind == SwitchKind::Demoted && !kReadsDemoted) {
        demotedSwitchSet(r.name);
        return r.dflt;
    }
    const char* v = std::getenv(r.name);
    return v ? parse(r, v) : r.dflt;
}

const char* typeOf(SwitchRule rule) {
    switch (rule) {
    case SwitchRule::OffOnZero:
    case SwitchRule::OnOnOne:
    case SwitchRule::Present: return "on/off";
    case SwitchRule::Int:
    case SwitchRule::IntMin1: return "integer";
    case SwitchRule::MiB: return "size";
    default: return "enumerated";
    }
}

}  // namespace

long long switchValue(Switch id) { return valueOf(kRows[static_cast<int>(id)]); }

Switches Switches::fromEnvironment() {
    Switches s;
#define X(field, type, name, kind, rule, dflt, path, doc) s.field = static_cast<type>(switchValue(Switch::field));
    EMF_SWITCH_TABLE(X)
#undef X
    return s;
}

std::string describeSwitches() {
    static const char* const ruleNames[] = {"OffOnZero", "OnOnOne", "Present", "Int", "IntMin1", "Lanes", "Flags012", "Priority", "MiB"};
    std::string out = "{\"debug_switches\": ";
    out += kReadsDemoted ? "true" : "false";
    out += ", \"switches\": [";
    bool first = true;
    for (const Row& r : kRows) {
        const bool demoted = r.kind == SwitchKind::Demoted;
        const long long value = valueOf(r);
        if (!first) out += ", ";
        first = false;
        // (names, rules and documentation lines hold no character JSON would want escaped)
        out += std::string("{\"name\": \"") + r.name + "\", \"field\": \"" + r.field + "\", \"kind\": \"" +
               (demoted ? "demoted" : "product") + "\", \"type\": \"" + typeOf(r.rule) + "\", \"rule\": \"" +
               ruleNames[static_cast<int>(r.rule)] + "\", \"default\": " + std::to_string(r.dflt) + ", \"read\": " +
               (demoted && !kReadsDemoted ? "false" : "true") + ", \"value\": " + std::to_string(value) + ", \"path\": " +
               (r.path ? "true" : "false") + ", \"doc\": \"" + r.doc + "\"}";
    }
    return out + "]}";
}

}  // namespace emf
