// Walks every layout function of gpyrn_amd/csrc/batch_layout.h (nothing else of the library is included) over small shapes
// -- one and three evaluations, q = 1 (no K_j^-1 tables), with and without mask entries, odd int counts, a fill program whose
// size is no multiple of 8 -- and checks, with the counts restated here: the size of the null-base walk is where the real
// walk ends, every range is aligned for its type, inside the block, and disjoint from the others; the per-sweep tables are one
// contiguous tail.  The one-tile slabs (walk_small): q = 1 and 3, reference and bound form, 1 and 17 evaluations, every offset
// against its formula written out.  Built and run by tests/test_batch_layout.py.
#include "batch_layout.h"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

struct Range { const char* name; uintptr_t at; size_t bytes, align; };
#define RANGE(ptr, count) Range{#ptr, (uintptr_t)(ptr), (size_t)(count) * sizeof(*(ptr)), alignof(decltype(*(ptr)))}

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void check(const char* what, const void* base, size_t bytes_null, size_t bytes_real, std::vector<Range> r)
{
    const uintptr_t b = (uintptr_t)base;
    CHECK(bytes_null == bytes_real, "%s: %zu bytes from the null walk, %zu from the real one", what, bytes_null, bytes_real);
    uintptr_t end = b;
    for (const Range& x : r) {
        CHECK(x.at % x.align == 0, "%s.%s is not aligned to %zu", what, x.name, x.align);
        CHECK(x.at >= b && x.at + x.bytes <= b + bytes_real, "%s.%s leaves the block", what, x.name);
        end = std::max(end, x.at + x.bytes);
    }
    CHECK(end == b + bytes_real, "%s: the ranges end at %zu of %zu bytes", what, (size_t)(end - b), bytes_real);
    r.erase(std::remove_if(r.begin(), r.end(), [](const Range& x) { return x.bytes == 0; }), r.end());
    std::sort(r.begin(), r.end(), [](const Range& x, const Range& y) { return x.at < y.at; });
    for (size_t i = 1; i < r.size(); ++i)
        CHECK(r[i - 1].at + r[i - 1].bytes <= r[i].at, "%s: %s and %s overlap", what, r[i - 1].name, r[i].name);
}

static std::vector<Range> ptr_ranges(const MidPtrTab& t, const MidShape& s)
{
    const size_t nslot = s.cap * s.G;
    return {RANGE(t.kptr, nslot), RANGE(t.kptr2, nslot), RANGE(t.setup, nslot * s.nb), RANGE(t.kinv, s.cap * (s.q - 1) * s.nb),
            RANGE(t.pred, nslot * s.nb), RANGE(t.diag, nslot), RANGE(t.node, s.cap * s.q * s.nb),
            RANGE(t.weight, s.cap * s.q * s.p * s.nb), RANGE(t.mask[0], s.cap * s.ne0 * s.nb), RANGE(t.mask[1], s.cap * s.ne1 * s.nb)};
}

static std::vector<Range> int_ranges(const MidIntTab& t, const MidShape& s)
{
    const size_t nslot = s.cap * s.G;
    return {RANGE(t.gp_setup, nslot), RANGE(t.ev_setup, nslot), RANGE(t.row_pred, nslot), RANGE(t.gp_node, s.cap * s.q),
            RANGE(t.ev_node, s.cap * s.q), RANGE(t.gp_weight, s.cap * s.q * s.p), RANGE(t.ev_weight, s.cap * s.q * s.p),
            RANGE(t.evals, s.cap)};
}

// a block of the size the null-base walk asks for, 64-byte aligned
struct Block {
    size_t bytes;
    void* at;
    explicit Block(size_t b) : bytes(b), at(aligned_alloc(64, (b + 63) / 64 * 64)) {}
    ~Block() { free(at); }
};

static void walk(const MidShape& s, size_t N, size_t program)
{
    const size_t nslot = s.cap * s.G, qp = s.q * s.p, ne = s.ne0 + s.ne1, state = (s.p + 1) * s.q * N, yv = s.p * N, hist = 12, lead = 4;
    {
        Block b(layout_count<char>(mid_ptr_tab, s));
        LayoutCursor c(b.at);
        const MidPtrTab t = mid_ptr_tab(c, s);
        check("mid_ptr_tab", b.at, b.bytes, c.at, ptr_ranges(t, s));
        CHECK(b.bytes == layout_count<double*>(mid_ptr_tab, s) * sizeof(double*), "mid_ptr_tab is no whole number of pointers");
        const MidPtrTab n = layout_at(nullptr, mid_ptr_tab, s);
        CHECK(n.kptr == nullptr && n.mask[1] == nullptr && n.end == nullptr, "a null base hands out pointers");
        // the set-up's tables first -- each ENDS at or ahead of node --, then ONE tail: node | weight | mask rows | end
        for (const Range& r : ptr_ranges(t, s))
            if (r.at < (uintptr_t)t.node) CHECK(r.at + r.bytes <= (uintptr_t)t.node, "set-up table %s reaches into the tail", r.name);
        CHECK(t.kptr == (double**)b.at && (char*)t.diag + nslot * sizeof(double*) == (char*)t.node, "the tail does not start behind diag");
        CHECK(t.weight == t.node + s.cap * s.q * s.nb && t.mask[0] == t.weight + s.cap * qp * s.nb &&
              t.mask[1] == t.mask[0] + s.cap * s.ne0 * s.nb && t.end == t.mask[1] + s.cap * s.ne1 * s.nb &&
              (char*)t.end == (char*)b.at + b.bytes, "the per-sweep pointer tables are not one contiguous tail");
    }
    {
        Block b(layout_count<char>(mid_int_tab, s));
        LayoutCursor c(b.at);
        const MidIntTab t = mid_int_tab(c, s);
        check("mid_int_tab", b.at, b.bytes, c.at, int_ranges(t, s));
        CHECK(layout_count<int>(mid_int_tab, s) == 3 * nslot + 2 * s.cap * s.q + 2 * s.cap * qp + s.cap, "mid_int_tab's count");
        CHECK(t.gp_node == t.gp_setup + 3 * nslot && t.end == t.evals + s.cap && (char*)t.end == (char*)b.at + b.bytes &&
              t.ev_node == t.gp_node + s.cap * s.q && t.gp_weight == t.ev_node + s.cap * s.q && t.evals == t.ev_weight + s.cap * qp,
              "the per-sweep int tables are not one contiguous tail");
    }
    {
        Block b(layout_count<char>(mid_pin_tab, s));
        LayoutCursor c(b.at);
        const MidPinTab t = mid_pin_tab(c, s);
        std::vector<Range> r = ptr_ranges(t.ptr, s), ri = int_ranges(t.ints, s);
        r.insert(r.end(), ri.begin(), ri.end());
        r.push_back(RANGE(t.lanes, s.cap * ne));
        check("mid_pin_tab", b.at, b.bytes, c.at, r);
        CHECK((size_t)(t.ptr.end - t.ptr.kptr) == layout_count<double*>(mid_ptr_tab, s) &&
              (size_t)(t.ints.end - t.ints.gp_setup) == layout_count<int>(mid_int_tab, s), "the image's tables differ from the device's");
    }
    {
        Block b(layout_count<char>(mid_pin_out, s.cap, s.G, state, lead));
        LayoutCursor c(b.at);
        const MidPinOut t = mid_pin_out(c, s.cap, s.G, state, lead);
        check("mid_pin_out", b.at, b.bytes, c.at,
              {RANGE(t.out4, lead * s.cap * 4), RANGE(t.info, 3 * nslot), RANGE(t.mu, s.cap * state), RANGE(t.var, s.cap * state)});
        CHECK((uintptr_t)t.mu % 64 == 0, "mid_pin_out.mu is not on a 64-byte boundary");
    }
    {
        Block b(layout_count<char>(small_pin_out, s.cap, s.G, state, hist));
        LayoutCursor c(b.at);
        const SmallPinOut t = small_pin_out(c, s.cap, s.G, state, hist);
        check("small_pin_out", b.at, b.bytes, c.at,
              {RANGE(t.ctl, s.cap * 4), RANGE(t.hist, s.cap * hist), RANGE(t.info, s.cap * 3 * s.G), RANGE(t.state, 4 * s.cap * state)});
        CHECK((uintptr_t)t.state % 64 == 0, "small_pin_out.state is not on a 64-byte boundary");
    }
    {
        Block b(layout_count<char>(batch_pin_in, s.cap, s.G, program, yv, state));
        LayoutCursor c(b.at);
        const BatchBufs t = batch_pin_in(c, s.cap, s.G, program, yv, state);
        check("batch_pin_in", b.at, b.bytes, c.at,
              {RANGE(t.programs, nslot * program), RANGE(t.yres, s.cap * yv), RANGE(t.variance, s.cap * yv),
               RANGE(t.mu, s.cap * state), RANGE(t.var, s.cap * state)});
    }
}

// The one-tile slabs (SmallSlab): the four blocks at the sizes small_batch_ensure allocates -- restated here --, every
// range inside its block and disjoint from the others, and every offset equal to the formula written out.
static void walk_small(size_t cap, size_t q, size_t p, size_t N, size_t ld, bool bound)
{
    const size_t G = q * (p + 1), nmat = bound ? 4 * G : 4 * G + q, nn = ld * ld, d = (p + 1) * q * N, pn = p * N;
    SmallSlab v{SmallShape{cap, G, q, p, N, ld, nmat}, nullptr, nullptr, nullptr, nullptr};
    CHECK(v.mats_count() == cap * nmat * nn && v.vecs_count() == cap * 7 * G * ld && v.state_count() == 4 * cap * d &&
          v.yv_count() == 2 * cap * pn, "small slab: the blocks' sizes");
    CHECK(v.per_eval() == nmat * nn + 7 * G * ld + 4 * d + 2 * pn && v.vec_pitch() == 7 * G * ld && v.d() == d && v.pn() == pn,
          "small slab: one evaluation's share");
    Block bm(v.mats_count() * sizeof(double)), bv(v.vecs_count() * sizeof(double)), bs(v.state_count() * sizeof(double)),
        by(v.yv_count() * sizeof(double));
    v.mats = (double*)bm.at; v.vecs = (double*)bv.at; v.states = (double*)bs.at; v.yv = (double*)by.at;
    std::vector<Range> rm, rv, rs, ry;
    for (size_t b = 0; b < cap; ++b) {
        double* const mb = v.mats + b * nmat * nn;
        for (size_t g = 0; g < G; ++g) {
            CHECK(v.K(b, g) == mb + g * nn && v.KLinv(b, g) == mb + (G + g) * nn && v.B(b, g) == mb + (2 * G + g) * nn &&
                  v.X(b, g) == mb + (3 * G + g) * nn, "small slab: the matrices of evaluation %zu, latent GP %zu", b, g);
            rm.push_back(RANGE(v.K(b, g), nn)); rm.push_back(RANGE(v.KLinv(b, g), nn));
            rm.push_back(RANGE(v.B(b, g), nn)); rm.push_back(RANGE(v.X(b, g), nn));
        }
        for (size_t j = 0; j < q && !bound; ++j) {
            CHECK(v.Kinv(b, j) == mb + (4 * G + j) * nn, "small slab: K^-1 of evaluation %zu, node %zu", b, j);
            rm.push_back(RANGE(v.Kinv(b, j), nn));
        }
        const SmallVec which[7] = {SV_D, SV_S, SV_PRED, SV_Z, SV_U, SV_CS, SV_CT};
        for (size_t w = 0; w < 7; ++w)
            for (size_t g = 0; g < G; ++g) {
                CHECK(v.vec(b, which[w], g) == v.vecs + b * 7 * G * ld + (w * G + g) * ld, "small slab: vector %zu of slot %zu", w, g);
                rv.push_back(RANGE(v.vec(b, which[w], g), ld));
            }
        for (size_t k = 0; k < 4; ++k) {
            CHECK(v.state(k, b) == v.states + (k * cap + b) * d && v.state_index(k, b) == k * cap + b, "small slab: state copy %zu", k);
            rs.push_back(RANGE(v.state(k, b), d));
        }
        CHECK(v.yres(b) == v.yv + b * pn && v.variance(b) == v.yv + (cap + b) * pn, "small slab: y - mean | variance");
        ry.push_back(RANGE(v.yres(b), pn)); ry.push_back(RANGE(v.variance(b), pn));
    }
    // (s and ct as the prediction's pitched copies read them: rows G + g and 6 G + g of an evaluation's 7 G)
    CHECK(v.vec(0, SV_S, 0) == v.vecs + G * ld && v.vec(0, SV_CT, 0) == v.vecs + 6 * G * ld, "small slab: where s and ct start");
    check("small slab mats", bm.at, bm.bytes, bm.bytes, rm);
    check("small slab vecs", bv.at, bv.bytes, bv.bytes, rv);
    check("small slab states", bs.at, bs.bytes, bs.bytes, rs);
    check("small slab yv", by.at, by.bytes, by.bytes, ry);
    CHECK(small_final_copy(0) == 0 && small_final_copy(1) == 2 && small_final_copy(2) == 0 && small_final_copy(7) == 2,
          "the copy of the last committed sweep: B after an odd trip count");
}

int main()
{
    int shapes = 0;
    for (size_t cap : {1, 17})
        for (size_t q : {1, 3})
            for (int bound = 0; bound < 2; ++bound) {
                walk_small(cap, q, 2, 45, 128, bound != 0);
                ++shapes;
            }
    for (size_t cap : {1, 3})
        for (size_t q : {1, 2})
            for (size_t p : {1, 2})
                for (size_t program : {200, 52})
                    for (int masked = 0; masked < 3; ++masked) {
                        walk(MidShape{cap, q * (p + 1), q, p, masked == 1 ? (size_t)1 : 0, masked ? q * p : 0, 4}, 45, program);
                        ++shapes;
                    }
    printf("%d shapes, %d failures\n", shapes, failures);
    return failures ? 1 : 0;
}
