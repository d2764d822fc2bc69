// bf_evt.cpp -- candidate events (include/dsabf.h: bf_evt_*; docs/EVENTS.md section 1): a streaming friends-of-friends grouping of
// the search's bf_sps_candidate records.  Host only, fp64, no GPU; a pure function of the sequence of feeds.
//
// What is kept between feeds: the open clusters' aggregates and their LIVE members (a0, a1, dm, cluster).  A member that can no
// longer link to anything a later feed brings is folded into its cluster's aggregate and forgotten, so the state is bounded by
// the candidates of a few pushes plus one beam bitmap per open cluster.
//
// One feed never looks at all pairs.  The live members and the new candidates are sorted by a0 and swept; behind the sweep, each
// trial keeps the member with the largest a1 seen so far.  B links to an earlier A of trial d iff b0 <= a1 + t_tol (a0 <= b0 <=
// b1 gives the other inequality), and all earlier members of one trial that reach b0 are linked to one another for the same
// reason -- so joining B to the ONE member of every trial within dm_tol that reaches furthest gives the same components as all
// pairs.  The cost is n log n for the sort plus n x (trials within dm_tol that hold a member).
#include <algorithm>
#include <cmath>
#include <new>
#include <numeric>
#include <set>
#include <vector>

#include "bf_runtime_internal.h"

namespace {

// best: larger snr; then smaller t_start, dm, beam, width
bool better(const bf_sps_candidate& a, const bf_sps_candidate& b)
{
    if (a.snr != b.snr) return a.snr > b.snr;
    if (a.t_start != b.t_start) return a.t_start < b.t_start;
    if (a.dm != b.dm) return a.dm < b.dm;
    if (a.beam != b.beam) return a.beam < b.beam;
    return a.width < b.width;
}

struct Cluster {
    bool has_coh = false, has_ib = false;
    bf_sps_candidate coh{}, ib{};       // the best member among the beams other than ib_beam, and among ib_beam's
    uint64_t t_lo = 0, t_hi = 0;
    int32_t dm_lo = 0, dm_hi = 0;
    int64_t n_members = 0;
    std::vector<uint64_t> beams;        // bitmap of the beams other than ib_beam, grown as needed ...
    std::set<int32_t> odd_beams;        // ... and the indices no sane bitmap holds (negative, or beyond 2^20)

    void add(const bf_sps_candidate& c, int32_t ib_beam)
    {
        const uint64_t a0 = c.t_start, a1 = c.t_start + (uint64_t)(c.width > 0 ? c.width - 1 : 0);
        if (!n_members) {
            t_lo = a0, t_hi = a1, dm_lo = dm_hi = c.dm;
        } else {
            t_lo = std::min(t_lo, a0), t_hi = std::max(t_hi, a1), dm_lo = std::min(dm_lo, c.dm), dm_hi = std::max(dm_hi, c.dm);
        }
        n_members++;
        if (ib_beam >= 0 && c.beam == ib_beam) {
            if (!has_ib || better(c, ib)) ib = c;
            has_ib = true;
            return;
        }
        if (!has_coh || better(c, coh)) coh = c;
        has_coh = true;
        if (c.beam < 0 || c.beam >= (1 << 20)) {
            odd_beams.insert(c.beam);
            return;
        }
        const size_t word = (size_t)c.beam / 64;
        if (beams.size() <= word) beams.resize(word + 1, 0);
        beams[word] |= (uint64_t)1 << (c.beam % 64);
    }
    void merge(const Cluster& o)
    {
        if (!o.n_members) return;
        if (!n_members) {
            *this = o;
            return;
        }
        t_lo = std::min(t_lo, o.t_lo), t_hi = std::max(t_hi, o.t_hi), dm_lo = std::min(dm_lo, o.dm_lo), dm_hi = std::max(dm_hi, o.dm_hi);
        n_members += o.n_members;
        if (o.has_coh && (!has_coh || better(o.coh, coh))) coh = o.coh;
        if (o.has_ib && (!has_ib || better(o.ib, ib))) ib = o.ib;
        has_coh = has_coh || o.has_coh;
        has_ib = has_ib || o.has_ib;
        if (beams.size() < o.beams.size()) beams.resize(o.beams.size(), 0);
        for (size_t w = 0; w < o.beams.size(); w++) beams[w] |= o.beams[w];
        odd_beams.insert(o.odd_beams.begin(), o.odd_beams.end());
    }
    bf_evt_event event(const bf_evt_options& o) const
    {
        bf_evt_event e{};
        e.best = has_coh ? coh : ib;
        e.t_lo = t_lo, e.t_hi = t_hi, e.dm_lo = dm_lo, e.dm_hi = dm_hi;
        e.n_members = (int32_t)std::min<int64_t>(n_members, INT32_MAX);
        size_t nb = odd_beams.size();
        for (uint64_t w : beams) nb += (size_t)__builtin_popcountll(w);
        e.n_beams = (int32_t)nb;
        e.snr_ib = has_ib ? ib.snr : 0.0;
        if (!has_coh) e.flags |= BF_EVT_IB_ONLY;
        if (e.n_beams > o.max_beams) e.flags |= BF_EVT_WIDE;
        const double bar = o.ib_ratio * e.best.snr;   // one multiply, one compare (the library is built without contraction)
        if (o.ib_beam >= 0 && (!has_coh || e.snr_ib >= bar)) e.flags |= BF_EVT_INCOHERENT;
        return e;
    }
};

struct Member {
    uint64_t a0, a1;
    int32_t dm;
    int32_t cluster;   // index into the open clusters; -1: a candidate of this feed
    int32_t cand;      // its index in the feed, -1: a live member from before
};

struct State {
    std::vector<Cluster> open;
    std::vector<Member> live;
};

int find(std::vector<int32_t>& parent, int x)
{
    while (parent[(size_t)x] != x) x = parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
    return x;
}

}  // namespace

struct bf_evt {
    bf_evt_options opt{};
    State st;
};

// One feed: `st` and the candidates -> the state behind it and the events that close.  `st` is left as it is: the caller commits
// the result only when the events fit.  close_all: nothing stays live (bf_evt_flush).
static void step(const bf_evt_options& o, const State& st, const bf_sps_candidate* cands, size_t n, uint64_t next_t, bool close_all, State& after,
                 std::vector<bf_evt_event>& closed)
{
    std::vector<Member> m(st.live);
    m.reserve(st.live.size() + n);
    for (size_t i = 0; i < n; i++) {
        const bf_sps_candidate& c = cands[i];
        m.push_back(Member{c.t_start, c.t_start + (uint64_t)(c.width > 0 ? c.width - 1 : 0), c.dm, -1, (int32_t)i});
    }
    const size_t M = m.size();
    std::vector<int32_t> parent(M);
    std::iota(parent.begin(), parent.end(), 0);
    auto unite = [&](int a, int b) {
        a = find(parent, a), b = find(parent, b);
        if (a != b) parent[(size_t)std::max(a, b)] = std::min(a, b);
    };
    // the live members of one open cluster belong together whatever this feed brings
    {
        std::vector<int32_t> first(st.open.size(), -1);
        for (size_t k = 0; k < st.live.size(); k++) {
            int32_t& f = first[(size_t)m[k].cluster];
            if (f < 0) f = (int32_t)k; else unite(f, (int)k);
        }
    }
    // the trials that hold a member, ascending: one bucket each
    std::vector<int32_t> trials(M);
    for (size_t k = 0; k < M; k++) trials[k] = m[k].dm;
    std::sort(trials.begin(), trials.end());
    trials.erase(std::unique(trials.begin(), trials.end()), trials.end());
    std::vector<int32_t> reach(trials.size(), -1);   // per bucket: the member behind the sweep with the largest a1
    std::vector<int32_t> order(M);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return m[(size_t)x].a0 != m[(size_t)y].a0 ? m[(size_t)x].a0 < m[(size_t)y].a0 : x < y; });
    const uint64_t t_tol = (uint64_t)o.t_tol;
    for (int32_t k : order) {
        const Member& b = m[(size_t)k];
        const int64_t lo = (int64_t)b.dm - o.dm_tol, hi = (int64_t)b.dm + o.dm_tol;
        size_t d = (size_t)(std::lower_bound(trials.begin(), trials.end(), lo, [](int32_t t, int64_t v) { return (int64_t)t < v; }) - trials.begin());
        size_t own = 0;
        for (; d < trials.size() && (int64_t)trials[d] <= hi; d++) {
            if (trials[d] == b.dm) own = d;
            const int32_t a = reach[d];
            if (a >= 0 && b.a0 - std::min(b.a0, t_tol) <= m[(size_t)a].a1) unite(a, k);   // b0 <= a1 + t_tol, without overflow
        }
        if (reach[own] < 0 || m[(size_t)reach[own]].a1 < b.a1) reach[own] = k;
    }
    // the components: every root gets a cluster, made of the open clusters and the new candidates it holds
    std::vector<int32_t> slot(M, -1);
    std::vector<Cluster> cl;
    std::vector<char> merged(st.open.size(), 0);
    for (size_t k = 0; k < M; k++) {
        const int r = find(parent, (int)k);
        if (slot[(size_t)r] < 0) {
            slot[(size_t)r] = (int32_t)cl.size();
            cl.emplace_back();
        }
        Cluster& c = cl[(size_t)slot[(size_t)r]];
        if (m[k].cand >= 0) {
            c.add(cands[m[k].cand], o.ib_beam);
        } else if (!merged[(size_t)m[k].cluster]) {
            merged[(size_t)m[k].cluster] = 1;
            c.merge(st.open[(size_t)m[k].cluster]);
        }
    }
    // who stays: a member is live while a1 + t_tol >= next_t - (max_width - 1)
    const uint64_t back = (uint64_t)(o.max_width - 1);
    const uint64_t limit = next_t > back ? next_t - back : 0;
    std::vector<int32_t> keep(cl.size(), -1);
    after.open.clear();
    after.live.clear();
    for (size_t k = 0; k < M && !close_all; k++) {
        if (m[k].a1 < limit - std::min(limit, t_tol)) continue;
        const int32_t c = slot[(size_t)find(parent, (int)k)];
        if (keep[(size_t)c] < 0) {
            keep[(size_t)c] = (int32_t)after.open.size();
            after.open.push_back(cl[(size_t)c]);
        }
        after.live.push_back(Member{m[k].a0, m[k].a1, m[k].dm, keep[(size_t)c], -1});
    }
    closed.clear();
    for (size_t c = 0; c < cl.size(); c++)
        if (keep[c] < 0) closed.push_back(cl[c].event(o));
    std::sort(closed.begin(), closed.end(), [](const bf_evt_event& a, const bf_evt_event& b) {
        if (a.best.t_start != b.best.t_start) return a.best.t_start < b.best.t_start;
        if (a.best.dm != b.best.dm) return a.best.dm < b.best.dm;
        return a.best.beam < b.best.beam;
    });
}

static int run(bf_evt* e, const bf_sps_candidate* cands, size_t n, uint64_t next_t, bool close_all, bf_evt_event* out, size_t max_out,
               size_t* n_out, const char* who)
{
    if (n_out) *n_out = 0;
    if (!e || !n_out || (n && !cands) || (max_out && !out)) return fail(BF_ERR_INVALID, "%s: NULL argument", who);
    if (n > (size_t)INT32_MAX / 2) return fail(BF_ERR_INVALID, "%s: %zu candidates in one feed", who, n);
    try {
        State after;
        std::vector<bf_evt_event> closed;
        step(e->opt, e->st, cands, n, next_t, close_all, after, closed);
        if (closed.size() > max_out)
            return fail(BF_ERR_INVALID, "%s: %zu events close and max_out is %zu; nothing was consumed", who, closed.size(), max_out);
        std::copy(closed.begin(), closed.end(), out);
        *n_out = closed.size();
        e->st.open.swap(after.open);
        e->st.live.swap(after.live);
    } catch (const std::bad_alloc&) {
        return fail(BF_ERR_DEVICE, "%s: out of host memory", who);
    }
    return BF_OK;
}

extern "C" {

void bf_evt_default_options(bf_evt_options* o)
{
    if (!o) return;
    o->t_tol = 0;
    o->dm_tol = 1;
    o->max_width = 128;
    o->max_beams = 4;
    o->ib_beam = -1;
    o->ib_ratio = 0.5;
}

int bf_evt_create(const bf_evt_options* o, bf_evt** out)
{
    if (!out) return fail(BF_ERR_INVALID, "out is NULL");
    *out = nullptr;
    bf_evt_options opt;
    bf_evt_default_options(&opt);
    if (o) opt = *o;
    if (opt.t_tol < 0 || opt.dm_tol < 0) return fail(BF_ERR_INVALID, "bf_evt_create: t_tol and dm_tol must be >= 0");
    if (opt.max_width < 1) return fail(BF_ERR_INVALID, "bf_evt_create: max_width must be >= 1");
    if (opt.max_beams < 0) return fail(BF_ERR_INVALID, "bf_evt_create: max_beams must be >= 0");
    if (!(opt.ib_ratio >= 0.0)) return fail(BF_ERR_INVALID, "bf_evt_create: ib_ratio must be a number >= 0");
    bf_evt* e = new (std::nothrow) bf_evt();
    if (!e) return fail(BF_ERR_DEVICE, "out of host memory");
    e->opt = opt;
    *out = e;
    return BF_OK;
}

int bf_evt_destroy(bf_evt* e)
{
    delete e;
    return BF_OK;
}

int bf_evt_feed(bf_evt* e, const bf_sps_candidate* cands, size_t n, uint64_t next_t, bf_evt_event* out, size_t max_out, size_t* n_out)
{
    return run(e, cands, n, next_t, false, out, max_out, n_out, "bf_evt_feed");
}

int bf_evt_flush(bf_evt* e, bf_evt_event* out, size_t max_out, size_t* n_out)
{
    return run(e, nullptr, 0, 0, true, out, max_out, n_out, "bf_evt_flush");
}

int bf_evt_open(const bf_evt* e) { return e ? (int)e->st.open.size() : BF_ERR_INVALID; }

}  // extern "C"
