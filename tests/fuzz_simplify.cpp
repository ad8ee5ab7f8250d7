// Stand-alone driver for the simplifying constructor of the native compiler
// (Lowerer::rule in mythril_amd/csrc/mg_compile.cpp), built with
// -fsanitize=address,undefined by tests/test_simplify.py.  It compiles random
// small DAGs that are dense in equal operands and boundary numerals (0, 1,
// all ones, the sign bit, 2^k, 2^k - 1) through the C ABI with a
// zero-initialised mgc_input (the pass on) at both register layouts, and once
// more with no_simplify set.  Every compile must end in MGC_OK, the pass
// must have folded something over the run and nothing with no_simplify.
// Host only.
//
// usage: fuzz_simplify <dags>
#include "mythcc.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

static std::vector<std::string> op_names() {
    std::vector<std::string> v;
    std::string all(mgc_source_ops());
    size_t p = 0;
    while (true) {
        size_t q = all.find('\n', p);
        v.push_back(all.substr(p, q == std::string::npos ? std::string::npos : q - p));
        if (q == std::string::npos) break;
        p = q + 1;
    }
    return v;
}

struct Dag {
    std::vector<int32_t> op, sort, width, dom, arg_off{0}, args, str, cval_off, cons, probes;
    std::vector<int64_t> id, p0, p1;
    std::vector<uint32_t> cval;
    std::string strings;
    int n_strings = 0;

    int add(int o, int s, int w, std::initializer_list<int> a, int name = -1) {
        op.push_back(o); sort.push_back(s); width.push_back(w); dom.push_back(0);
        id.push_back((int64_t)op.size());
        for (int x : a) args.push_back(x);
        arg_off.push_back((int32_t)args.size());
        p0.push_back(0); p1.push_back(0); str.push_back(name); cval_off.push_back(-1);
        return (int)op.size() - 1;
    }
};

static long meta_int(const char* meta, const char* key) {
    const char* p = std::strstr(meta, key);
    return p ? std::atol(p + std::strlen(key)) : -1;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    int n_dags = std::atoi(argv[1]);
    std::vector<std::string> names = op_names();
    auto code = [&names](const char* n) {
        for (size_t i = 0; i < names.size(); i++) if (names[i] == n) return (int)i;
        std::abort();
    };
    const char* bin_names[] = {"bvadd", "bvsub", "bvmul", "bvand", "bvor", "bvxor", "bvudiv", "bvurem",
                               "bvsdiv", "bvsrem", "bvsmod", "bvshl", "bvlshr", "bvashr"};
    const char* cmp_names[] = {"bvult", "bvule", "bvugt", "bvuge", "bvslt", "bvsle", "bvsgt", "bvsge",
                               "bvumul_noovfl", "="};
    const char* bool_names[] = {"and", "or", "xor", "=>"};
    std::vector<int> bins, cmps, bools;
    for (auto n : bin_names) bins.push_back(code(n));
    for (auto n : cmp_names) cmps.push_back(code(n));
    for (auto n : bool_names) bools.push_back(code(n));
    const int BVNUM = code("bvnum"), VAR = code("var"), ITE = code("ite"), NOT = code("not"),
              BVNEG = code("bvneg"), BVNOT = code("bvnot"), TRUE_ = code("true"), FALSE_ = code("false");
    const int widths[] = {1, 8, 33, 64, 255, 256};

    std::mt19937_64 rng(0x73696d70);
    long ok = 0, errors = 0, folded = 0, folded_off = 0, appended = 0;
    for (int d = 0; d < n_dags; d++) {
        Dag g;
        const int w = widths[rng() % 6];
        const int nl = (w + 31) / 32;
        auto pick = [&rng](size_t n) { return (size_t)(rng() % n); };
        std::vector<int> bv, bo;
        for (int v = 0; v < 3; v++) {
            std::string nm = "v" + std::to_string(v);
            g.strings += nm; g.strings.push_back('\0');
            bv.push_back(g.add(VAR, MGC_SORT_BV, w, {}, g.n_strings++));
        }
        g.strings += "c"; g.strings.push_back('\0');
        bo.push_back(g.add(VAR, MGC_SORT_BOOL, 1, {}, g.n_strings++));
        auto numeral = [&]() {
            std::vector<uint32_t> l((size_t)nl, 0);
            int k = (int)pick((size_t)w);
            switch (rng() % 7) {
            case 0: break;                                           // 0
            case 1: l[0] = 1; break;
            case 2: for (auto& x : l) x = 0xFFFFFFFFu; break;        // all ones
            case 3: l[(size_t)((w - 1) / 32)] = 1u << ((w - 1) % 32); break;   // the sign bit
            case 4: l[(size_t)(k / 32)] = 1u << (k % 32); break;     // 2^k
            case 5:                                                   // 2^(k+1) - 1
                for (int b = 0; b <= k; b++) l[(size_t)(b / 32)] |= 1u << (b % 32);
                break;
            default: for (auto& x : l) x = (uint32_t)rng(); break;
            }
            if (w % 32) l.back() &= (1u << (w % 32)) - 1;
            int n = g.add(BVNUM, MGC_SORT_BV, w, {});
            g.cval_off[(size_t)n] = (int32_t)g.cval.size();
            g.cval.insert(g.cval.end(), l.begin(), l.end());
            return n;
        };
        int n_ops = 20 + (int)pick(60);
        for (int k = 0; k < n_ops; k++) {
            // operands from the last few values, the same one twice a third of the time
            auto recent = [&](std::vector<int>& v) { return v[v.size() - 1 - pick(v.size() < 6 ? v.size() : 6)]; };
            int a = recent(bv), b = rng() % 3 == 0 ? a : recent(bv);
            switch (rng() % 10) {
            case 0: case 1: bv.push_back(numeral()); break;
            case 2: case 3: case 4: bv.push_back(g.add(bins[pick(bins.size())], MGC_SORT_BV, w, {a, b})); break;
            case 5: case 6: bo.push_back(g.add(cmps[pick(cmps.size())], MGC_SORT_BOOL, 1, {a, b})); break;
            case 7: bv.push_back(g.add(ITE, MGC_SORT_BV, w, {recent(bo), a, b})); break;
            case 8: {
                int x = recent(bo), y = rng() % 3 == 0 ? x : recent(bo);
                int r = (int)(rng() % 7);
                if (r < 4) bo.push_back(g.add(bools[(size_t)r], MGC_SORT_BOOL, 1, {x, y}));
                else if (r == 4) bo.push_back(g.add(NOT, MGC_SORT_BOOL, 1, {x}));
                else bo.push_back(g.add(r == 5 ? TRUE_ : FALSE_, MGC_SORT_BOOL, 1, {}));
                break;
            }
            default: bv.push_back(g.add(rng() % 2 ? BVNEG : BVNOT, MGC_SORT_BV, w, {a})); break;
            }
        }
        for (size_t i = 1; i < bo.size(); i++) if (rng() % 3 == 0 || i + 1 == bo.size()) g.cons.push_back(bo[i]);
        for (size_t i = 3; i < bv.size(); i++) if (rng() % 4 == 0) g.probes.push_back(bv[i]);

        const long errors_before = errors;
        for (int variant = 0; variant < 3; variant++) {
            mgc_input in;
            std::memset(&in, 0, sizeof in);
            in.n_nodes = (int32_t)g.op.size();
            in.op = g.op.data(); in.sort = g.sort.data(); in.width = g.width.data(); in.dom = g.dom.data();
            in.id = g.id.data(); in.arg_off = g.arg_off.data(); in.args = g.args.data();
            in.p0 = g.p0.data(); in.p1 = g.p1.data(); in.str = g.str.data();
            in.cval_off = g.cval_off.data(); in.cval = g.cval.data(); in.n_cval = (int32_t)g.cval.size();
            in.strings = g.strings.data(); in.n_strings = g.n_strings;
            in.n_string_bytes = (int32_t)g.strings.size();
            in.n_cons = (int32_t)g.cons.size(); in.cons = g.cons.data();
            in.n_probes = (int32_t)g.probes.size(); in.probes = g.probes.data();
            in.default_entries = 2;
            in.nreg = variant == 1 ? 11 : 16;
            in.remat_mode = MGC_REMAT_SCRATCH; in.remat_k = 2; in.keep_clean = 1;
            in.leaf_pools = variant == 1;
            if (variant == 2) in.no_simplify = 1;
            mgc_result* res = nullptr;
            int rc = mgc_compile(&in, &res);
            if (rc != MGC_OK) {
                std::fprintf(stderr, "dag %d variant %d: rc %d: %s\n", d, variant, rc, mgc_error(res));
                errors++;
            } else {
                long f = meta_int(mgc_meta(res), "\"folded\":");
                long ap = meta_int(mgc_meta(res), "\"appended\":");
                int32_t n_ins = 0, rows = 0, ncv = 0;
                (void)mgc_code(res, &n_ins);
                (void)mgc_table(res, &rows, &ncv);
                if (f < 0 || ap < 0 || n_ins <= 0 || ncv > rows || (variant == 2 && ap != 0)) errors++;
                if (variant == 2) folded_off += f;
                else { folded += f; appended += ap; }
            }
            mgc_free(res);
        }
        ok += errors == errors_before;
    }
    std::printf("{\"dags\": %d, \"ok\": %ld, \"errors\": %ld, \"folded\": %ld, \"appended\": %ld, "
                "\"folded_off\": %ld}\n", n_dags, ok, errors, folded, appended, folded_off);
    return errors ? 1 : 0;
}
