// tapstark_air.hpp -- header-only C++ capture of an AIR into the constraint tape ts_air_compile takes.
//
// The compiled-language counterpart of tap-stark_amd/air.py, mirroring how the reference turns an
// `Air::eval` body into symbolic constraints:
//   SymbolicVariable / Entry      uni-stark/src/symbolic_variable.rs:9-38
//   SymbolicExpression            uni-stark/src/symbolic_expression.rs:12-61 (degree rules :41-61)
//   SymbolicAirBuilder            uni-stark/src/symbolic_builder.rs:68-148
//   get_symbolic_constraints      uni-stark/src/symbolic_builder.rs:52-64
//   FilteredAirBuilder            p3-air (when_first_row / when_transition / when_last_row)
// Write `eval(ts::air::Builder&)` the way the reference writes `eval(&self, builder: &mut AB)`, then
// hand `builder.tape()` to ts_air_compile.  No dependency beyond the standard library and tapstark.h beside it (whose
// ts_scan_spec the Scan builder at the end fills).
#pragma once
#include <stdint.h>

#include <map>
#include <stdexcept>
#include <tuple>
#include <vector>

#include "tapstark.h"

namespace ts {
namespace air {

constexpr uint32_t P = 0x78000001u;  // basic/src/field/mod.rs:45
constexpr uint32_t TAPE_MAGIC = 0x54415354u;
enum Op : uint32_t { CONST = 0, MAIN = 1, PUBLIC = 2, IS_FIRST = 3, IS_LAST = 4, IS_TRANSITION = 5,
                     ADD = 6, SUB = 7, NEG = 8, MUL = 9,
                     PREP = 10,  // version-2 tapes: Entry::Preprocessed { offset }, symbolic_variable.rs:9-15
                     // version-3 tapes (build-defined: challenge-phase columns, include/tapstark.h)
                     AUX = 11, CHALLENGE = 12, EXPOSED = 13 };
constexpr uint32_t EF_W = 11;  // EF4 = F[x] / (x^4 - 11)

class Builder;

// a node of the constraint DAG (hash-consed per builder: shared sub-expressions are emitted once)
class Expr {
public:
    Expr() = default;
    Expr(Builder* b, uint32_t id) : b_(b), id_(id) {}
    uint32_t id() const { return id_; }
    Builder* builder() const { return b_; }

private:
    Builder* b_ = nullptr;
    uint32_t id_ = 0;
};

class Filtered;
struct ExtExpr;

class Builder {
public:
    // preprocessed_width > 0: an AIR with preprocessed (fixed) columns, symbolic_builder.rs:68-99; its variables
    // come first, as there, and the tape is version 2
    // aux_width / n_challenges / n_exposed > 0: an AIR with challenge-phase columns; their variables come last and
    // the tape is version 3
    Builder(uint32_t width, uint32_t num_public_values, uint32_t preprocessed_width = 0, uint32_t aux_width = 0,
            uint32_t n_challenges = 0, uint32_t n_exposed = 0)
        : width_(width), n_public_(num_public_values), prep_width_(preprocessed_width), aux_width_(aux_width),
          n_challenges_(n_challenges), n_exposed_(n_exposed) {
        for (uint32_t off = 0; off < 2; off++)
            for (uint32_t c = 0; c < preprocessed_width; c++) prep_[off].push_back(node(PREP, off, c, 1));
        for (uint32_t off = 0; off < 2; off++)
            for (uint32_t c = 0; c < width; c++) rows_[off].push_back(node(MAIN, off, c, 1));
        for (uint32_t i = 0; i < num_public_values; i++) public_.push_back(node(PUBLIC, i, 0, 0));
        for (uint32_t off = 0; off < 2; off++)
            for (uint32_t c = 0; c < aux_width; c++) aux_[off].push_back(node(AUX, off, c, 1));
        for (uint32_t k = 0; k < 4 * n_challenges; k++) challenge_words_.push_back(node(CHALLENGE, k, 0, 0));
        for (uint32_t e = 0; e < n_exposed; e++) exposed_.push_back(node(EXPOSED, e, 0, 0));
    }
    // builder.main().row_slice(0 | 1)
    const std::vector<Expr>& local() const { return rows_[0]; }
    const std::vector<Expr>& next() const { return rows_[1]; }
    // PairBuilder::preprocessed().row_slice(offset), symbolic_builder.rs:144-148
    const std::vector<Expr>& preprocessed(uint32_t offset) const { return prep_[offset & 1]; }
    const std::vector<Expr>& public_values() const { return public_; }
    // the challenge-phase trace's row slices, challenge k as an extension element, the exposed base words
    const std::vector<Expr>& aux(uint32_t offset) const { return aux_[offset & 1]; }
    ExtExpr challenge(uint32_t k) const;
    const std::vector<Expr>& exposed() const { return exposed_; }
    void assert_zero_ext(const ExtExpr& x);  // FOUR base constraints
    Expr constant(uint64_t v) { return node(CONST, (uint32_t)(v % P), 0, 0); }
    Expr is_first_row() { return node(IS_FIRST, 0, 0, 1); }    // symbolic_expression.rs:45
    Expr is_last_row() { return node(IS_LAST, 0, 0, 1); }      // :46
    Expr is_transition() { return node(IS_TRANSITION, 0, 0, 0); }  // :47 (window size 2)
    void assert_zero(Expr x) { constraints_.push_back(x.id()); }  // symbolic_builder.rs:136-138
    void assert_eq(Expr x, Expr y);
    Filtered when(Expr c);
    Filtered when_first_row();
    Filtered when_last_row();
    Filtered when_transition();

    // symbolic_builder.rs:15-50
    uint32_t max_constraint_degree() const {
        uint32_t d = 0;
        for (uint32_t c : constraints_) d = degs_[c] > d ? degs_[c] : d;
        return d;
    }
    uint32_t log_quotient_degree() const {
        uint32_t d = max_constraint_degree();
        if (d < 2) d = 2;
        uint32_t k = 0;
        while ((1u << k) < d - 1) k++;  // log2_ceil(d - 1)
        return k;
    }
    // [magic, version, width, n_public, n_nodes, n_constraints, nodes (op, a, b)..., constraint ids...];
    // version 2 (preprocessed_width > 0) has the preprocessed width as a seventh header word; version 3 (aux
    // columns, challenges or exposed words) a ten-word header: ..., preprocessed_width, aux_width, n_challenges,
    // n_exposed
    std::vector<uint32_t> tape() const {
        const bool v3 = aux_width_ || n_challenges_ || n_exposed_;
        std::vector<uint32_t> t = {TAPE_MAGIC, v3 ? 3u : prep_width_ ? 2u : 1u, width_, n_public_,
                                   (uint32_t)nodes_.size(), (uint32_t)constraints_.size()};
        if (v3) t.insert(t.end(), {prep_width_, aux_width_, n_challenges_, n_exposed_});
        else if (prep_width_) t.push_back(prep_width_);
        for (auto& n : nodes_) {
            t.push_back(std::get<0>(n));
            t.push_back(std::get<1>(n));
            t.push_back(std::get<2>(n));
        }
        t.insert(t.end(), constraints_.begin(), constraints_.end());
        return t;
    }

    Expr node(uint32_t op, uint32_t a, uint32_t b, uint32_t deg) {
        const auto key = std::make_tuple(op, a, b);
        auto it = cse_.find(key);
        if (it != cse_.end()) return Expr(this, it->second);
        const uint32_t id = (uint32_t)nodes_.size();
        nodes_.push_back(key);
        degs_.push_back(deg);
        cse_[key] = id;
        return Expr(this, id);
    }
    uint32_t degree(Expr e) const { return degs_[e.id()]; }

private:
    uint32_t width_, n_public_, prep_width_, aux_width_, n_challenges_, n_exposed_;
    std::vector<std::tuple<uint32_t, uint32_t, uint32_t>> nodes_;
    std::vector<uint32_t> degs_;
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, uint32_t> cse_;
    std::vector<uint32_t> constraints_;
    std::vector<Expr> rows_[2], prep_[2], public_, aux_[2], challenge_words_, exposed_;
};

// degree rules: symbolic_expression.rs:137 (add), :182 (sub), :227 (mul)
inline Expr operator+(Expr x, Expr y) {
    Builder* b = x.builder();
    const uint32_t dx = b->degree(x), dy = b->degree(y);
    return b->node(ADD, x.id(), y.id(), dx > dy ? dx : dy);
}
inline Expr operator-(Expr x, Expr y) {
    Builder* b = x.builder();
    const uint32_t dx = b->degree(x), dy = b->degree(y);
    return b->node(SUB, x.id(), y.id(), dx > dy ? dx : dy);
}
inline Expr operator-(Expr x) { return x.builder()->node(NEG, x.id(), 0, x.builder()->degree(x)); }
inline Expr operator*(Expr x, Expr y) {
    Builder* b = x.builder();
    return b->node(MUL, x.id(), y.id(), b->degree(x) + b->degree(y));
}
inline Expr operator+(Expr x, uint64_t c) { return x + x.builder()->constant(c); }
inline Expr operator-(Expr x, uint64_t c) { return x - x.builder()->constant(c); }
inline Expr operator*(Expr x, uint64_t c) { return x * x.builder()->constant(c); }

// An extension-field expression: four coefficients over x^4 - 11.  assert_zero_ext emits FOUR base constraints,
// so an extension-valued constraint is an ordinary constraint of the tape language.  Every operator builds its
// nodes in one fixed order (the Python ExtExpr's), so both front ends give the same tape.
struct ExtExpr {
    Expr c[4];
    static ExtExpr from_base(Expr x) {
        const Expr zero = x.builder()->constant(0);
        return ExtExpr{{x, zero, zero, zero}};
    }
    static ExtExpr from_base(Builder& b, uint64_t v) {
        const Expr x = b.constant(v);
        return from_base(x);
    }
    ExtExpr mul_base(Expr x) const {
        ExtExpr r;
        for (int k = 0; k < 4; k++) r.c[k] = c[k] * x;
        return r;
    }
};
inline ExtExpr operator+(const ExtExpr& x, const ExtExpr& y) {
    ExtExpr r;
    for (int k = 0; k < 4; k++) r.c[k] = x.c[k] + y.c[k];
    return r;
}
inline ExtExpr operator-(const ExtExpr& x, const ExtExpr& y) {
    ExtExpr r;
    for (int k = 0; k < 4; k++) r.c[k] = x.c[k] - y.c[k];
    return r;
}
inline ExtExpr operator-(const ExtExpr& x, Expr y) { return x - ExtExpr::from_base(y); }
inline ExtExpr operator-(const ExtExpr& x) {
    ExtExpr r;
    for (int k = 0; k < 4; k++) r.c[k] = -x.c[k];
    return r;
}
inline ExtExpr operator*(const ExtExpr& x, Expr y) { return x.mul_base(y); }
// r_k = sum_{i+j=k} a_i b_j + 11 sum_{i+j=k+4} a_i b_j
inline ExtExpr operator*(const ExtExpr& x, const ExtExpr& y) {
    ExtExpr r;
    for (int k = 0; k < 4; k++) {
        std::vector<Expr> lo, hi;
        for (int i = 0; i <= k; i++) lo.push_back(x.c[i] * y.c[k - i]);
        for (int i = k + 1; i < 4; i++) hi.push_back(x.c[i] * y.c[k + 4 - i]);
        Expr acc = lo[0];
        for (size_t t = 1; t < lo.size(); t++) acc = acc + lo[t];
        if (!hi.empty()) {
            Expr h = hi[0];
            for (size_t t = 1; t < hi.size(); t++) h = h + hi[t];
            const Expr w = h.builder()->constant(EF_W);
            const Expr hw = h * w;
            acc = acc + hw;
        }
        r.c[k] = acc;
    }
    return r;
}
inline ExtExpr Builder::challenge(uint32_t k) const {
    return ExtExpr{{challenge_words_.at(4 * k), challenge_words_.at(4 * k + 1), challenge_words_.at(4 * k + 2),
                    challenge_words_.at(4 * k + 3)}};
}
inline void Builder::assert_zero_ext(const ExtExpr& x) {
    for (int k = 0; k < 4; k++) assert_zero(x.c[k]);
}

// p3-air FilteredAirBuilder: when(c).assert_zero(x) => assert_zero(c * x)
class Filtered {
public:
    Filtered(Builder* b, Expr cond) : b_(b), cond_(cond) {}
    void assert_zero(Expr x) { b_->assert_zero(cond_ * x); }
    void assert_zero_ext(const ExtExpr& x) {
        for (int k = 0; k < 4; k++) assert_zero(x.c[k]);
    }
    void assert_eq(Expr x, Expr y) { assert_zero(x - y); }
    void assert_one(Expr x) { assert_zero(x - 1); }
    Filtered when(Expr c) { return Filtered(b_, cond_ * c); }

private:
    Builder* b_;
    Expr cond_;
};
inline void Builder::assert_eq(Expr x, Expr y) { assert_zero(x - y); }
inline Filtered Builder::when(Expr c) { return Filtered(this, c); }
inline Filtered Builder::when_first_row() { return when(is_first_row()); }
inline Filtered Builder::when_last_row() { return when(is_last_row()); }
inline Filtered Builder::when_transition() { return when(is_transition()); }


// ---- LogUp over the main trace (include/tapstark.h, csrc/logup.hip): the constraints that match the aux columns
// ts_logup_aux_build makes, from the same interaction spec.  Two challenges gamma, beta; interaction i has
// d_i = gamma + sum_j beta^j v_ij and the fraction m_i / d_i; group g pairs interactions 2g and 2g+1; aux columns
// 4g .. 4g+3 hold the group's sum h_g, the last four the exclusive running sum phi, the four exposed words S:
//   h_g d_a d_b - m_a d_b - m_b d_a = 0 (degree 3; h_g d_a - m_a = 0 for an odd last group)
//   is_first phi = 0,  is_transition (phi' - phi - sum_g h_g) = 0,  is_last (phi + sum_g h_g - S) = 0
// No d is zero, so these determine the aux matrix from trace and challenges.  The statement "S = 0" is the
// caller's to check after ts_verify_aux.
struct LogUpTerm {
    uint32_t kind;   // 0: the canonical constant `value`; 1: main column `value`, local row; 2: preprocessed
                     // column `value`, local row (a lookup against a fixed table: ts_logup_aux_build_pre)
    uint32_t value;
};
struct LogUpInteraction {
    LogUpTerm multiplicity;
    std::vector<LogUpTerm> values;
};
class LogUp {
public:
    static constexpr uint32_t n_challenges = 2, n_exposed = 4;
    explicit LogUp(std::vector<LogUpInteraction> interactions) : its_(std::move(interactions)) {
        if (its_.empty()) throw std::invalid_argument("LogUp: no interactions");
    }
    const std::vector<LogUpInteraction>& interactions() const { return its_; }
    uint32_t n_groups() const { return ((uint32_t)its_.size() + 1) / 2; }
    uint32_t aux_width() const { return 4 * (n_groups() + 1); }

    void eval(Builder& b) const {
        const auto& main = b.local();
        const auto &aux = b.aux(0), &aux_next = b.aux(1);
        const ExtExpr gamma = b.challenge(0), beta = b.challenge(1);
        const auto& prep = b.preprocessed(0);
        auto term = [&](LogUpTerm t) {
            return t.kind == 0 ? b.constant(t.value) : t.kind == 2 ? prep.at(t.value) : main.at(t.value);
        };
        size_t n_pow = 0;
        for (auto& it : its_) n_pow = it.values.size() > n_pow ? it.values.size() : n_pow;
        std::vector<ExtExpr> beta_pow{ExtExpr::from_base(b, 1)};
        for (size_t j = 1; j < n_pow; j++) {
            const ExtExpr next = beta_pow.back() * beta;
            beta_pow.push_back(next);
        }
        std::vector<ExtExpr> dens;
        std::vector<Expr> mults;
        for (auto& it : its_) {
            ExtExpr d = gamma;
            for (size_t j = 0; j < it.values.size(); j++) {
                const Expr v = term(it.values[j]);
                const ExtExpr t = beta_pow[j].mul_base(v);
                d = d + t;
            }
            dens.push_back(d);
            mults.push_back(term(it.multiplicity));
        }
        const uint32_t G = n_groups();
        auto ext_at = [](const std::vector<Expr>& row, uint32_t first) {
            return ExtExpr{{row.at(first), row.at(first + 1), row.at(first + 2), row.at(first + 3)}};
        };
        ExtExpr total;
        for (uint32_t g = 0; g < G; g++) {
            const ExtExpr h = ext_at(aux, 4 * g);
            const size_t ia = 2 * g, ib = 2 * g + 1;
            const ExtExpr hd = h * dens[ia];
            if (ib < dens.size()) {
                const ExtExpr t1 = hd * dens[ib];
                const ExtExpr t2 = dens[ib].mul_base(mults[ia]);
                const ExtExpr t3 = t1 - t2;
                const ExtExpr t4 = dens[ia].mul_base(mults[ib]);
                b.assert_zero_ext(t3 - t4);
            } else {
                b.assert_zero_ext(hd - mults[ia]);
            }
            total = g == 0 ? h : total + h;
        }
        const ExtExpr phi = ext_at(aux, 4 * G), phi_next = ext_at(aux_next, 4 * G), S = ext_at(b.exposed(), 0);
        {
            Filtered f = b.when_first_row();
            f.assert_zero_ext(phi);
        }
        {
            Filtered f = b.when_transition();
            const ExtExpr step = phi_next - phi;
            f.assert_zero_ext(step - total);
        }
        {
            Filtered f = b.when_last_row();
            const ExtExpr end = phi + total;
            f.assert_zero_ext(end - S);
        }
    }

#ifdef TAPSTARK_H
    // The ts_logup_mult_spec (needs tapstark.h included first) that fills the multiplicity column of the table-side
    // interaction `table` -- its multiplicity term must be a main column: that column receives the result, its
    // values are the table's tuple -- from the interactions `lookups` (their multiplicity terms are the weights),
    // negated so that the filled trace balances.  `spec` points into the object's own storage: keep the object
    // alive and where it is over the call.
    struct MultSpec {
        std::vector<ts_logup_term> table, lookups, weights;
        ts_logup_mult_spec spec;
        MultSpec() = default;
        MultSpec(const MultSpec& o) : table(o.table), lookups(o.lookups), weights(o.weights), spec(o.spec) { repoint(); }
        MultSpec& operator=(const MultSpec& o) {
            table = o.table, lookups = o.lookups, weights = o.weights, spec = o.spec;
            repoint();
            return *this;
        }
        void repoint() { spec.table = table.data(), spec.lookups = lookups.data(), spec.weights = weights.data(); }
    };
    MultSpec mult_spec(size_t table, const std::vector<size_t>& lookups) const {
        const LogUpInteraction& t = its_.at(table);
        if (t.multiplicity.kind != 1)
            throw std::invalid_argument("LogUp::mult_spec: the table interaction's multiplicity must be a main column");
        if (lookups.empty()) throw std::invalid_argument("LogUp::mult_spec: no lookups");
        MultSpec m;
        for (const LogUpTerm& v : t.values) m.table.push_back(ts_logup_term{v.kind, v.value});
        for (size_t i : lookups) {
            const LogUpInteraction& l = its_.at(i);
            if (i == table || l.values.size() != t.values.size())
                throw std::invalid_argument("LogUp::mult_spec: a lookup is the table or has another number of values");
            for (const LogUpTerm& v : l.values) m.lookups.push_back(ts_logup_term{v.kind, v.value});
            m.weights.push_back(ts_logup_term{l.multiplicity.kind, l.multiplicity.value});
        }
        m.spec.struct_size = sizeof(ts_logup_mult_spec);
        m.spec.n_values = (uint32_t)t.values.size();
        m.spec.n_lookups = (uint32_t)lookups.size();
        m.spec.out_column = t.multiplicity.value;
        m.spec.negate = 1;
        m.repoint();
        return m;
    }
#endif

private:
    std::vector<LogUpInteraction> its_;
};

// ---- row programs for ts_matrix_derive (include/tapstark.h "derived columns"): the counterpart of
// tap-stark_amd/derive.py, node for node -- nothing is shared or folded, an integer operand becomes a CONST node where
// it is met, so a program written statement by statement in the same order gives the same tape words in both.  (C++
// leaves the order in which the two sides of an operator are evaluated open: write one operation per statement where
// the words matter.)  Nothing is checked here; ts_derive_check is the judge.
class Derive;

class DExpr {
public:
    DExpr(Derive* b, uint32_t id) : b_(b), id_(id) {}
    uint32_t id() const { return id_; }
    Derive* builder() const { return b_; }
    inline DExpr inv() const;
    inline DExpr is_zero() const;
    inline DExpr lt(DExpr o) const;
    inline DExpr bits(uint32_t shift, uint32_t n) const;  // (x >> shift) & (2^n - 1) on the canonical integer

private:
    Derive* b_;
    uint32_t id_;
};

class Derive {
public:
    enum Op : uint32_t { CONST = 0, COL = 1, IS_FIRST = 3, IS_LAST = 4, IS_TRANSITION = 5, ADD = 6, SUB = 7, NEG = 8,
                         MUL = 9, ROW = 32, INV = 33, IS_ZERO = 34, LT = 35, BITS = 36, AND = 37, XOR = 38 };
    static constexpr uint32_t MAGIC = 0x52454454u;  // "TDER"

    explicit Derive(uint32_t src_width) : src_width_(src_width) {}
    DExpr node(uint32_t op, uint32_t a, uint32_t b) {
        nodes_.insert(nodes_.end(), {op, a, b});
        return DExpr(this, (uint32_t)(nodes_.size() / 3 - 1));
    }
    DExpr constant(uint64_t v) { return node(CONST, (uint32_t)(v % P), 0); }
    DExpr col(uint32_t c) { return node(COL, 0, c); }
    DExpr next(uint32_t c) { return node(COL, 1, c); }
    DExpr prev(uint32_t c) { return node(COL, 2, c); }
    DExpr row() { return node(ROW, 0, 0); }
    DExpr is_first_row() { return node(IS_FIRST, 0, 0); }
    DExpr is_last_row() { return node(IS_LAST, 0, 0); }
    DExpr is_transition() { return node(IS_TRANSITION, 0, 0); }
    void output(DExpr x, uint32_t dst_column) { outputs_.insert(outputs_.end(), {x.id(), dst_column}); }
    std::vector<uint32_t> tape() const {
        std::vector<uint32_t> t = {MAGIC, 1, src_width_, (uint32_t)(nodes_.size() / 3), (uint32_t)(outputs_.size() / 2)};
        t.insert(t.end(), nodes_.begin(), nodes_.end());
        t.insert(t.end(), outputs_.begin(), outputs_.end());
        return t;
    }

protected:
    uint32_t src_width_;
    std::vector<uint32_t> nodes_, outputs_;
};

// ---- row programs with carried state for the iterate form of ts_matrix_derive (include/tapstark.h "iterated
// columns"): the counterpart of tap-stark_amd/iterate.py, a Derive whose tape is a TITR tape.  carry(init) makes one
// register and gives the expression that reads it -- its value from BEFORE this row, init on a group's first row;
// set_carry says what it holds after a row.  A carry that was never set names node 0xFFFFFFFF and is refused.
class Iterate : public Derive {
public:
    enum GroupOp : uint32_t { CARRY = 40, STEP = 41, IS_GROUP_FIRST = 42, IS_GROUP_LAST = 43 };
    static constexpr uint32_t MAGIC = 0x52544954u;  // "TITR"
    static constexpr uint32_t NO_RESET = 0xFFFFFFFFu;

    explicit Iterate(uint32_t src_width, uint32_t reset_column = NO_RESET, uint32_t max_group_rows = 1024)
        : Derive(src_width), reset_column_(reset_column), max_group_rows_(max_group_rows) {}
    DExpr carry(uint64_t init = 0) {
        carries_.insert(carries_.end(), {0xFFFFFFFFu, (uint32_t)(init % P)});
        return node(CARRY, (uint32_t)(carries_.size() / 2 - 1), 0);
    }
    // `carry` is what carry() returned
    void set_carry(DExpr carry, DExpr x) { carries_[2 * nodes_[3 * carry.id() + 1]] = x.id(); }
    DExpr step() { return node(STEP, 0, 0); }
    DExpr is_group_first() { return node(IS_GROUP_FIRST, 0, 0); }
    DExpr is_group_last() { return node(IS_GROUP_LAST, 0, 0); }
    std::vector<uint32_t> tape() const {
        std::vector<uint32_t> t = {MAGIC, 1, src_width_, (uint32_t)(nodes_.size() / 3), (uint32_t)(outputs_.size() / 2),
                                   (uint32_t)(carries_.size() / 2), reset_column_, max_group_rows_};
        t.insert(t.end(), nodes_.begin(), nodes_.end());
        t.insert(t.end(), outputs_.begin(), outputs_.end());
        t.insert(t.end(), carries_.begin(), carries_.end());
        return t;
    }

private:
    uint32_t reset_column_, max_group_rows_;
    std::vector<uint32_t> carries_;  // {node, init} per carry
};

inline DExpr DExpr::inv() const { return b_->node(Derive::INV, id_, 0); }
inline DExpr DExpr::is_zero() const { return b_->node(Derive::IS_ZERO, id_, 0); }
inline DExpr DExpr::lt(DExpr o) const { return b_->node(Derive::LT, id_, o.id()); }
inline DExpr DExpr::bits(uint32_t shift, uint32_t n) const { return b_->node(Derive::BITS, id_, shift | n << 8); }
inline DExpr operator+(DExpr x, DExpr y) { return x.builder()->node(Derive::ADD, x.id(), y.id()); }
inline DExpr operator-(DExpr x, DExpr y) { return x.builder()->node(Derive::SUB, x.id(), y.id()); }
inline DExpr operator*(DExpr x, DExpr y) { return x.builder()->node(Derive::MUL, x.id(), y.id()); }
inline DExpr operator&(DExpr x, DExpr y) { return x.builder()->node(Derive::AND, x.id(), y.id()); }
inline DExpr operator^(DExpr x, DExpr y) { return x.builder()->node(Derive::XOR, x.id(), y.id()); }
inline DExpr operator-(DExpr x) { return x.builder()->node(Derive::NEG, x.id(), 0); }
inline DExpr operator+(DExpr x, uint64_t c) { return x + x.builder()->constant(c); }
inline DExpr operator-(DExpr x, uint64_t c) { return x - x.builder()->constant(c); }
inline DExpr operator*(DExpr x, uint64_t c) { return x * x.builder()->constant(c); }
inline DExpr operator+(uint64_t c, DExpr x) { return x.builder()->constant(c) + x; }
inline DExpr operator-(uint64_t c, DExpr x) { return x.builder()->constant(c) - x; }
inline DExpr operator*(uint64_t c, DExpr x) { return x.builder()->constant(c) * x; }

// ---- scans for ts_matrix_scan (include/tapstark.h "scanned columns"): the counterpart of tap-stark_amd/scan.py.  A
// term is a constant (reduced mod p here) or Scan::col(c); add() appends one recurrence y[i] = a[i] y[i-1] + b[i] and
// spec() is the struct the call takes.  Nothing is checked here: the call is the judge (a ninth scan is counted, not
// stored, so that it is refused).
class Scan {
public:
    static ts_scan_term constant(uint64_t v) { return ts_scan_term{0, (uint32_t)(v % P)}; }
    static ts_scan_term col(uint32_t c) { return ts_scan_term{1, c}; }

    explicit Scan(uint32_t out_width = 0) : spec_() {
        spec_.struct_size = (uint32_t)sizeof(ts_scan_spec);
        spec_.out_width = out_width;
    }
    Scan& add(uint32_t dst, ts_scan_term a, ts_scan_term b, uint32_t init = 0, uint32_t reset = TS_SCAN_NO_RESET,
              bool exclusive = false) {
        if (spec_.n_columns < TS_SCAN_MAX_COLUMNS)
            spec_.columns[spec_.n_columns] = ts_scan_column{a, b, init, reset, dst, exclusive ? (uint32_t)TS_SCAN_EXCLUSIVE : 0u};
        spec_.n_columns++;
        return *this;
    }
    // y[i] = y[i-1] + src[i][column]
    Scan& running_sum(uint32_t column, uint32_t dst, uint32_t reset = TS_SCAN_NO_RESET) {
        return add(dst, constant(1), col(column), 0, reset);
    }
    // y[i] = src[i][column] * y[i-1], from 1
    Scan& running_product(uint32_t column, uint32_t dst, uint32_t reset = TS_SCAN_NO_RESET) {
        return add(dst, col(column), constant(0), 1, reset);
    }
    const ts_scan_spec& spec() const { return spec_; }

private:
    ts_scan_spec spec_;
};

// ---- specs for ts_matrix_collect_rows (include/tapstark.h "collected rows"): the counterpart of
// tap-stark_amd/collect.py, word for word.  A term is Collect::constant(v) (reduced mod p here), Collect::col(c) or
// Collect::row(); a selector is Collect::always() or Collect::col(c).  emit() appends one emitter and tape() is the
// word tape the call takes.  Nothing is checked here; ts_collect_check is the judge.
class Collect {
public:
    struct Term {
        uint32_t kind, value;
    };
    static constexpr uint32_t MAGIC = 0x4C4F4354u;  // "TCOL"
    static Term constant(uint64_t v) { return Term{0, (uint32_t)(v % P)}; }
    static Term col(uint32_t c) { return Term{1, c}; }
    static Term row() { return Term{2, 0}; }
    static Term always() { return Term{0, 1}; }

    // a pad row shorter than out_width is filled with zeros
    Collect(std::vector<uint32_t> src_widths, uint32_t out_width, std::vector<uint32_t> pad = {})
        : src_widths_(std::move(src_widths)), out_width_(out_width), pad_(std::move(pad)) {
        pad_.resize(out_width_, 0);
    }
    Collect& emit(uint32_t source, Term when, const std::vector<Term>& terms) {
        records_.insert(records_.end(), {source, when.kind, when.value});
        for (const Term& t : terms) records_.insert(records_.end(), {t.kind, t.value});
        n_emitters_++;
        return *this;
    }
    std::vector<uint32_t> tape() const {
        std::vector<uint32_t> t = {MAGIC, 1, (uint32_t)src_widths_.size(), n_emitters_, out_width_};
        t.insert(t.end(), src_widths_.begin(), src_widths_.end());
        t.insert(t.end(), pad_.begin(), pad_.end());
        t.insert(t.end(), records_.begin(), records_.end());
        return t;
    }

private:
    std::vector<uint32_t> src_widths_;
    uint32_t out_width_, n_emitters_ = 0;
    std::vector<uint32_t> pad_, records_;
};

// ---- specs for the group form of ts_matrix_collect_rows (include/tapstark.h "grouped rows"): the counterpart of
// tap-stark_amd/group.py, word for word.  A key is Group::constant(v) (reduced mod p here) or Group::col(c); the selector
// Group::always() or Group::col(c); an output term Group::constant(v), Group::first(c), Group::last(c),
// Group::first_row(), Group::last_row(), Group::count(), Group::total(c), Group::least(c), Group::greatest(c) or
// Group::index().  tape() is the word tape the three collect calls take.  Nothing is checked here; ts_collect_check is
// the judge.
class Group {
public:
    struct Term {
        uint32_t kind, value;
    };
    static constexpr uint32_t MAGIC = 0x50524754u;  // "TGRP"
    static Term constant(uint64_t v) { return Term{0, (uint32_t)(v % P)}; }
    static Term col(uint32_t c) { return Term{1, c}; }  // as a key or the selector: column c; as an output term: first(c)
    static Term always() { return Term{0, 1}; }
    static Term first(uint32_t c) { return Term{1, c}; }
    static Term last(uint32_t c) { return Term{2, c}; }
    static Term first_row() { return Term{3, 0}; }
    static Term last_row() { return Term{4, 0}; }
    static Term count() { return Term{5, 0}; }
    static Term total(uint32_t c) { return Term{6, c}; }
    static Term least(uint32_t c) { return Term{7, c}; }
    static Term greatest(uint32_t c) { return Term{8, c}; }
    static Term index() { return Term{9, 0}; }

    // a pad row shorter than out_width is filled with zeros
    Group(uint32_t src_width, uint32_t out_width, std::vector<Term> keys, Term when = Term{0, 1},
          std::vector<uint32_t> pad = {})
        : src_width_(src_width), out_width_(out_width), keys_(std::move(keys)), when_(when), pad_(std::move(pad)) {
        pad_.resize(out_width_, 0);
    }
    Group& terms(const std::vector<Term>& terms) {
        terms_ = terms;
        return *this;
    }
    std::vector<uint32_t> tape() const {
        std::vector<uint32_t> t = {MAGIC, 1, src_width_, out_width_, (uint32_t)keys_.size(), when_.kind, when_.value};
        for (const Term& k : keys_) t.insert(t.end(), {k.kind, k.value});
        t.insert(t.end(), pad_.begin(), pad_.end());
        for (const Term& k : terms_) t.insert(t.end(), {k.kind, k.value});
        return t;
    }

private:
    uint32_t src_width_, out_width_;
    std::vector<Term> keys_;
    Term when_;
    std::vector<uint32_t> pad_;
    std::vector<Term> terms_;
};

// ---- specs for ts_matrix_expand_rows (include/tapstark.h "expanded rows"): the counterpart of
// tap-stark_amd/expand.py, word for word.  A term is Expand::constant(v) (reduced mod p here), Expand::col(c),
// Expand::row(), Expand::inner(), Expand::remaining(), Expand::first(), Expand::last() or Expand::stepped(c, step);
// count() and when() take Expand::col(c), count() also Expand::times(n).  tape() is the word tape the call takes.
// Nothing is checked here; ts_expand_check is the judge.
class Expand {
public:
    struct Term {
        uint32_t kind, value, step;
    };
    static constexpr uint32_t MAGIC = 0x50584554u;  // "TEXP"
    static Term constant(uint64_t v) { return Term{0, (uint32_t)(v % P), 0}; }
    static Term col(uint32_t c) { return Term{1, c, 0}; }
    static Term row() { return Term{2, 0, 0}; }
    static Term inner() { return Term{3, 0, 0}; }
    static Term remaining() { return Term{4, 0, 0}; }
    static Term first() { return Term{5, 0, 0}; }
    static Term last() { return Term{6, 0, 0}; }
    static Term stepped(uint32_t c, uint64_t step = 1) { return Term{7, c, (uint32_t)(step % P)}; }
    static Term times(uint32_t n) { return Term{0, n, 0}; }  // a constant count
    static Term always() { return Term{0, 1, 0}; }

    // a pad row shorter than out_width is filled with zeros
    Expand(uint32_t src_width, uint32_t out_width, uint32_t max_count, std::vector<uint32_t> pad = {})
        : src_width_(src_width), out_width_(out_width), max_count_(max_count), pad_(std::move(pad)) {
        pad_.resize(out_width_, 0);
    }
    Expand& count(Term t) {
        count_ = t;
        return *this;
    }
    Expand& when(Term t) {
        when_ = t;
        return *this;
    }
    Expand& terms(const std::vector<Term>& terms) {
        terms_ = terms;
        return *this;
    }
    std::vector<uint32_t> tape() const {
        std::vector<uint32_t> t = {MAGIC, 1, src_width_, out_width_, when_.kind, when_.value, count_.kind, count_.value,
                                   max_count_};
        t.insert(t.end(), pad_.begin(), pad_.end());
        for (const Term& x : terms_) t.insert(t.end(), {x.kind, x.value, x.step});
        return t;
    }

private:
    uint32_t src_width_, out_width_, max_count_;
    Term when_ = {0, 1, 0}, count_ = {0, 1, 0};
    std::vector<uint32_t> pad_;
    std::vector<Term> terms_;
};

// ---- specs for ts_matrix_join_rows (include/tapstark.h "joined rows"): the counterpart of tap-stark_amd/join.py.  It
// owns the arrays a ts_join_spec points to: spec() is valid until the next call of a builder method and as long as the
// Join lives.  A key term is Join::constant(v) (reduced mod p here) or Join::col(c).  Nothing is checked here;
// ts_join_check is the judge.
class Join {
public:
    static ts_logup_term constant(uint64_t v) { return ts_logup_term{0, (uint32_t)(v % P)}; }
    static ts_logup_term col(uint32_t c) { return ts_logup_term{1, c}; }

    explicit Join(uint32_t flags = 0, uint64_t table_rows = 0) : flags_(flags), table_rows_(table_rows) {}
    Join& key(ts_logup_term on_src, ts_logup_term on_table) {
        src_keys_.push_back(on_src);
        table_keys_.push_back(on_table);
        return *this;
    }
    Join& when(ts_logup_term t) {
        when_ = t;
        return *this;
    }
    Join& fetch(uint32_t table_column, uint32_t dst_column, uint32_t default_word = 0) {
        table_columns_.push_back(table_column);
        dst_columns_.push_back(dst_column);
        defaults_.push_back(default_word);
        return *this;
    }
    const ts_join_spec* spec() {
        spec_ = ts_join_spec{(uint32_t)sizeof(ts_join_spec), (uint32_t)src_keys_.size(), src_keys_.data(),
                             table_keys_.data(), when_, (uint32_t)table_columns_.size(), table_columns_.data(),
                             dst_columns_.data(), defaults_.data(), flags_, table_rows_};
        return &spec_;
    }

private:
    uint32_t flags_;
    uint64_t table_rows_;
    ts_logup_term when_ = {0, 1};
    std::vector<ts_logup_term> src_keys_, table_keys_;
    std::vector<uint32_t> table_columns_, dst_columns_, defaults_;
    ts_join_spec spec_ = {};
};

}  // namespace air
}  // namespace ts
