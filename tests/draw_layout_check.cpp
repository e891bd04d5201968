// Walks the draw pass's scratch layout (gpyrn_amd/csrc/batch_layout.h draw_scratch; nothing else of the library is included)
// over small shapes -- one and three evaluations, one and several blocks of t* (ns below, at and above ld), one tile and a
// ragged second tile of t*, one draw and more draws than a tile, an odd p -- and checks, with the counts restated here: the
// size of the null-base walk is where the real walk ends, every range is aligned for its type (the matrices to 256 bytes),
// inside the block and disjoint from the others; the shape's padded sizes and block count; the four pointer tables are one
// contiguous run (the pass uploads them with one copy); every row block of W, every matrix and every row the pass addresses
// lies inside its range; the two ranges that are used twice are large enough for their second use.  Built and run by
// tests/test_draw_layout.py; stands alone, so it can be built with -fsanitize=address,undefined.
#include "batch_layout.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

struct Range { const char* name; uintptr_t at; size_t bytes, align; };
#define RANGE(ptr, count, align) Range{#ptr, (uintptr_t)(ptr), (size_t)(count) * sizeof(*(ptr)), (size_t)(align)}

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void walk(size_t evals, size_t G, size_t p, size_t ld, size_t ns, size_t nd)
{
    const size_t nb = 4;
    const DrawShape s = draw_shape(evals, G, p, ld, ns, nd, nb);
    const size_t ns_pad = (ns + 127) / 128 * 128, nd_pad = (nd + 127) / 128 * 128, nblk = (ns + ld - 1) / ld, slots = evals * G;
    CHECK(s.slots == slots && s.evals == evals && s.p == p && s.ld == ld && s.ns == ns && s.nd == nd && s.nb == nb, "the shape's counts");
    CHECK(s.ns_pad == ns_pad && s.nd_pad == nd_pad && s.nblk == nblk, "the shape's padded sizes: %zu %zu %zu", s.ns_pad, s.nd_pad, s.nblk);
    CHECK(ns_pad >= ns && ns_pad - ns < 128 && nd_pad >= nd && nd_pad - nd < 128 && nblk * ld >= ns && (nblk - 1) * ld < ns, "padding");
    const size_t bytes = layout_count<char>(draw_scratch, s);
    void* const block = aligned_alloc(256, (bytes + 255) / 256 * 256);
    memset(block, 0, bytes);
    LayoutCursor c(block);
    const DrawScratch d = draw_scratch(c, s);
    CHECK(c.at == bytes, "%zu bytes from the null walk, %zu from the real one", bytes, c.at);
    const DrawScratch n = layout_at(nullptr, draw_scratch, s);
    CHECK(!n.W && !n.C && !n.F && !n.X && !n.Z && !n.LZ && !n.kss && !n.mean && !n.pvar && !n.out && !n.ts && !n.blk && !n.kblk &&
          !n.cs && !n.lz, "a null base hands out pointers");
    const size_t nn = ns_pad * ns_pad, nz = nd_pad * ns_pad, nw = ns_pad * ld;
    CHECK(d.nn() == nn && d.z_count() == nz && d.w_count() == nw, "one slot's share of the matrices");
    std::vector<Range> r = {RANGE(d.W, slots * nw, 256), RANGE(d.C, slots * nn, 256), RANGE(d.F, slots * nn, 256),
                            RANGE(d.X, slots * nn, 256), RANGE(d.Z, slots * nz, 256), RANGE(d.LZ, slots * nz, 256),
                            RANGE(d.kss, slots * ns_pad, 256), RANGE(d.mean, slots * ns_pad, 8), RANGE(d.pvar, slots * ns_pad, 8),
                            RANGE(d.out, evals * p * nd * ns, 256), RANGE(d.ts, ns, 8), RANGE(d.blk, nblk * slots * nb, 256),
                            RANGE(d.kblk, slots, 8), RANGE(d.cs, slots, 8), RANGE(d.lz, slots, 8)};
    const uintptr_t b = (uintptr_t)block;
    uintptr_t end = b;
    for (const Range& x : r) {
        CHECK(x.at % x.align == 0, "%s is not aligned to %zu", x.name, x.align);
        CHECK(x.at >= b && x.at + x.bytes <= b + bytes, "%s leaves the block", x.name);
        end = std::max(end, x.at + x.bytes);
    }
    CHECK(end == b + bytes, "the ranges end at %zu of %zu bytes", (size_t)(end - b), bytes);
    std::sort(r.begin(), r.end(), [](const Range& x, const Range& y) { return x.at < y.at; });
    for (size_t i = 1; i < r.size(); ++i)
        CHECK(r[i - 1].at + r[i - 1].bytes <= r[i].at, "%s and %s overlap", r[i - 1].name, r[i].name);
    // the per-slot share the header's comment and include/gprn_hip.h promise: ns_pad ld + 3 ns_pad^2 + 2 nd_pad ns_pad doubles
    CHECK((char*)d.kss - (char*)d.W >= (ptrdiff_t)(slots * (nw + 3 * nn + 2 * nz) * sizeof(double)) &&
          (char*)d.kss - (char*)d.W < (ptrdiff_t)(slots * (nw + 3 * nn + 2 * nz) * sizeof(double) + 6 * 256), "the matrices' share");
    // ONE run of pointers: [nblk][slots][nb] | kblk | cs | lz, as batch_draw_pass's one copy writes it
    CHECK(d.kblk == d.blk + nblk * slots * nb && d.cs == d.kblk + slots && d.lz == d.cs + slots &&
          (char*)(d.lz + slots) == (char*)block + bytes, "the pointer tables are not one contiguous tail");
    // what the pass addresses.  Row block b of a slot's W starts at row b ld and has the block's padded rows; a block's rows of
    // k**, mean* and var* start at t0 = b ld of the slot's ns_pad
    for (size_t sl = 0; sl < slots; ++sl) {
        double* const W = d.W + sl * nw;
        for (size_t k = 0; k < nblk; ++k) {
            const size_t t0 = k * ld, nsb = std::min(ld, ns - t0), nsb_pad = (nsb + 127) / 128 * 128;
            CHECK(W + k * ld * ld + nsb_pad * ld <= d.W + (sl + 1) * nw, "W: row block %zu of slot %zu leaves the slot's share", k, sl);
            CHECK(t0 + nsb_pad <= ns_pad, "rows: block %zu leaves a slot's rows", k);
            CHECK(nsb_pad <= ld, "a block has more rows than the driver's ld x ld buffer");
        }
    }
    {
        const size_t t0 = (nblk - 1) * ld;
        CHECK(t0 + (std::min(ld, ns - t0) + 127) / 128 * 128 == ns_pad, "the last block does not end at ns_pad: rows of W would stay unwritten");
    }
    // second uses: the caller's normals [slot][nd][ns] in LZ, the latent draws [slot][nd][ns] in Z
    CHECK(slots * nd * ns <= slots * nz, "the unpadded normals do not fit LZ");
    // (touch every byte through the typed pointers: a sanitizer build sees an overrun of the allocation)
    for (size_t i = 0; i < slots * nw; ++i) d.W[i] = 1.0;
    for (size_t i = 0; i < slots * nn; ++i) d.C[i] = d.F[i] = d.X[i] = 2.0;
    for (size_t i = 0; i < slots * nz; ++i) d.Z[i] = d.LZ[i] = 3.0;
    for (size_t i = 0; i < slots * ns_pad; ++i) d.kss[i] = d.mean[i] = d.pvar[i] = 4.0;
    for (size_t i = 0; i < evals * p * nd * ns; ++i) d.out[i] = 5.0;
    for (size_t i = 0; i < ns; ++i) d.ts[i] = 6.0;
    for (size_t i = 0; i < (nblk * nb + 3) * slots; ++i) d.blk[i] = nullptr;
    CHECK(d.W[slots * nw - 1] == 1.0 && d.X[slots * nn - 1] == 2.0 && d.LZ[slots * nz - 1] == 3.0 && d.pvar[slots * ns_pad - 1] == 4.0 &&
          d.out[evals * p * nd * ns - 1] == 5.0 && d.ts[ns - 1] == 6.0, "a range was overwritten by its neighbour");
    free(block);
}

int main()
{
    int shapes = 0;
    for (size_t evals : {1, 3})
        for (size_t ld : {128, 384})
            for (size_t ns : {1, 128, 129, 300, 385})
                for (size_t nd : {1, 5, 129})
                    for (size_t p : {1, 3}) {
                        walk(evals, p + 1, p, ld, ns, nd);
                        ++shapes;
                    }
    printf("%d shapes, %d failures\n", shapes, failures);
    return failures ? 1 : 0;
}
