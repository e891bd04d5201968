// Host check of gpyrn_amd/csrc/device_mem.h (tests/test_device_mem.py compiles and runs it; no GPU, no HIP): the four raw
// functions over malloc / free with a switch that makes the n-th allocation fail, then DeviceOwner and DevBuf through every
// path -- release, release twice, the destructor, ensure below / at / above capacity, and every allocation of a sequence of
// eight failing in turn.  Under -fsanitize=address,undefined a leak, a double free or a use after free ends the run.
#include "device_mem.h"

#include <stdio.h>
#include <stdlib.h>

std::atomic<long long> g_mem_live{0}, g_mem_made{0};
static long long g_calls = 0, g_fail_at = 0;       // the g_fail_at-th allocation from now fails (0: none)
static long long g_dev_live = 0, g_pin_live = 0;   // by kind: a buffer must go back through the function of its kind

static int raw_alloc(void** p, size_t bytes, std::string* err, long long* kind, int code, const char* what)
{
    *p = nullptr;
    if (bytes == 0 || (g_fail_at && ++g_calls == g_fail_at)) {
        if (err) *err = std::string(what) + ": out of memory";
        return code;
    }
    *p = malloc(bytes);
    *kind += 1; g_mem_live += 1; g_mem_made += 1;
    return GPRN_OK;
}
int mem_dev_alloc(void** p, size_t bytes, std::string* err) { return raw_alloc(p, bytes, err, &g_dev_live, GPRN_E_NOMEM, "hipMalloc"); }
int mem_pin_alloc(void** p, size_t bytes, std::string* err) { return raw_alloc(p, bytes, err, &g_pin_live, GPRN_E_HIP, "hipHostMalloc"); }
void mem_dev_free(void* p) { if (p) { free(p); g_dev_live -= 1; g_mem_live -= 1; } }
void mem_pin_free(void* p) { if (p) { free(p); g_pin_live -= 1; g_mem_live -= 1; } }

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)
static void fail_nth(long long n) { g_calls = 0; g_fail_at = n; }
struct Ctx { std::string err; };                   // what the library's callers pass: anything with an `err`

static void owner_paths()
{
    const long long live0 = g_mem_live, made0 = g_mem_made;
    Ctx c;
    {
        DeviceOwner own;
        double *a = nullptr, *z = nullptr; int* b = nullptr; char* h = nullptr;
        CHECK(own.alloc(&c, &a, 10) == GPRN_OK && a);
        CHECK(own.alloc(&b, 3, &c.err) == GPRN_OK && b);
        CHECK(own.alloc(&c, &z, 0) == GPRN_OK && z);            // (a zero count is one element)
        CHECK(own.pin(&c, &h, 64) == GPRN_OK && h);
        a[9] = 1.0; b[2] = 2; z[0] = 3.0; h[63] = 4;
        CHECK(g_mem_live == live0 + 4 && g_dev_live == 3 && g_pin_live == 1 && !own.empty());
        own.release();
        CHECK(g_mem_live == live0 && own.empty());
        own.release();                                          // twice
        CHECK(g_mem_live == live0 && g_dev_live == 0 && g_pin_live == 0);
        CHECK(own.alloc(&c, &a, 5) == GPRN_OK && own.pin(&c, &h, 8) == GPRN_OK);     // usable again; the destructor frees these
        CHECK(g_mem_live == live0 + 2);
    }
    CHECK(g_mem_live == live0 && g_mem_made == made0 + 6);
}

template <typename T>
static void buf_paths(bool pinned)
{
    const long long live0 = g_mem_live, made0 = g_mem_made;
    std::string err;
    {
        DevBuf<T> b(pinned);
        CHECK(b.ensure(0, &err) == GPRN_OK && !b.p && b.cap == 0 && g_mem_made == made0);
        CHECK(b.ensure(8, &err) == GPRN_OK && b.p && b.cap == 8);
        b.p[7] = T(1);
        T* const first = b.p;
        CHECK(b.ensure(5, &err) == GPRN_OK && b.p == first && b.cap == 8);       // below
        CHECK(b.ensure(8, &err) == GPRN_OK && b.p == first && b.cap == 8);       // at
        CHECK(g_mem_made == made0 + 1);
        CHECK(b.ensure(9, &err) == GPRN_OK && b.p && b.cap == 9);                // above: freed, then allocated
        b.p[8] = T(2);
        CHECK(g_mem_made == made0 + 2 && g_mem_live == live0 + 1);
        CHECK((pinned ? g_pin_live : g_dev_live) == 1 && (pinned ? g_dev_live : g_pin_live) == 0);
        fail_nth(1);
        const int rc = b.ensure(100, &err);                                     // a grow that fails: empty ...
        fail_nth(0);
        CHECK(rc == (pinned ? GPRN_E_HIP : GPRN_E_NOMEM) && !b.p && b.cap == 0 && !err.empty() && g_mem_live == live0);
        CHECK(b.ensure(4, &err) == GPRN_OK && b.p && b.cap == 4);                // ... and usable again
        b.p[3] = T(3);
        b.release();
        CHECK(!b.p && b.cap == 0 && g_mem_live == live0);
        b.release();                                                            // twice
        CHECK(b.ensure(2, &err) == GPRN_OK && g_mem_live == live0 + 1);          // the destructor frees this one
    }
    CHECK(g_mem_live == live0 && g_dev_live == 0 && g_pin_live == 0);
}

// eight allocations -- owner device, owner pinned and a DevBuf of each kind, twice over; the n-th fails, n = 1 .. 8, and 9: none
static void failing_sequence()
{
    for (long long n = 1; n <= 9; ++n) {
        const long long live0 = g_mem_live, made0 = g_mem_made;
        Ctx c;
        {
            DeviceOwner own;
            DevBuf<double> dbuf;
            DevBuf<int> pbuf(true);
            double* a0 = nullptr; int* a4 = nullptr; char *h1 = nullptr, *h5 = nullptr;
            int rc[8];
            fail_nth(n);
            rc[0] = own.alloc(&c, &a0, 16);
            rc[1] = own.pin(&c, &h1, 32);
            rc[2] = dbuf.ensure(4, &c.err); const void* const g2 = dbuf.p;
            rc[3] = pbuf.ensure(4, &c.err); const void* const g3 = pbuf.p;
            rc[4] = own.alloc(&c, &a4, 0);
            rc[5] = own.pin(&c, &h5, 1);
            rc[6] = dbuf.ensure(40, &c.err); const void* const g6 = dbuf.p;    // (after a failed first grow: usable again)
            rc[7] = pbuf.ensure(40, &c.err); const void* const g7 = pbuf.p;
            fail_nth(0);
            const void* const got[8] = {a0, h1, g2, g3, a4, h5, g6, g7};
            long long ok = 0;
            for (int i = 0; i < 8; ++i) {
                const bool failed = i + 1 == n;
                CHECK(failed ? rc[i] != GPRN_OK && !got[i] : rc[i] == GPRN_OK && got[i]);
                ok += !failed;
            }
            CHECK(g_mem_made == made0 + ok);
            // a DevBuf whose grow failed is empty and usable again
            if (n == 7) { CHECK(!dbuf.p && dbuf.cap == 0 && dbuf.ensure(3, &c.err) == GPRN_OK && dbuf.p && dbuf.cap == 3); dbuf.p[2] = 1.0; }
            if (n == 8) { CHECK(!pbuf.p && pbuf.cap == 0 && pbuf.ensure(3, &c.err) == GPRN_OK && pbuf.p && pbuf.cap == 3); pbuf.p[2] = 1; }
            if (n <= 8) CHECK(!c.err.empty());
            own.release();                                      // the owner releases clean; the buffers go with the scope
            CHECK(own.empty());
        }
        CHECK(g_mem_live == live0 && g_dev_live == 0 && g_pin_live == 0);
        CHECK(g_mem_made >= made0);
    }
}

int main()
{
    const long long live0 = g_mem_live;
    long long made = g_mem_made;
    owner_paths();
    CHECK(g_mem_made >= made); made = g_mem_made;
    buf_paths<double>(false);
    buf_paths<int>(true);
    CHECK(g_mem_made >= made); made = g_mem_made;
    failing_sequence();
    CHECK(g_mem_made >= made && g_mem_live == live0);
    printf("device_mem_check: %lld allocations made, %lld live, %d failures\n", (long long)g_mem_made, (long long)g_mem_live, failures);
    return failures ? 1 : 0;
}
