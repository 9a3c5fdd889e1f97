// The owner type of csrc/hipbuf.h on the host alone: Owned over a counting fake
// free function (no HIP call is made).  Every handle must be freed exactly
// once whatever is moved, reset or destroyed.  make check-hipbuf builds this
// plain and under ASan + UBSan (tests/test_hipbuf.py).
#include <cstdio>
#include <map>
#include <utility>
#include <vector>

#include "hipbuf.h"

namespace {

std::map<int *, int> g_freed;  // handle -> times freed
int g_failures = 0;

int fake_free(int *p)
{
    ++g_freed[p];
    return 0;
}

using Fake = tspgpu::Owned<int *, fake_free>;

int g_cells[16];

Fake make(int k, size_t cap)
{
    Fake f;
    f.p = &g_cells[k];
    f.cap = cap;
    return f;
}

int freed(int k) { return g_freed.count(&g_cells[k]) ? g_freed[&g_cells[k]] : 0; }

void expect(bool ok, const char *what)
{
    if (ok) return;
    std::printf("FAIL: %s\n", what);
    ++g_failures;
}

}  // namespace

int main()
{
    {  // move construction: the source is null with capacity 0 and frees nothing
        Fake a = make(0, 10);
        Fake b(std::move(a));
        expect(a.p == nullptr && a.cap == 0, "move construction empties the source");
        expect(b.p == &g_cells[0] && b.cap == 10, "move construction carries handle and capacity");
        expect(freed(0) == 0, "move construction frees nothing");
    }
    expect(freed(0) == 1, "handle 0 freed once, by the move's target");
    {  // move assignment: the target's old handle goes, the source is emptied
        Fake a = make(1, 1), b = make(2, 2);
        b = std::move(a);
        expect(freed(2) == 1 && freed(1) == 0, "move assignment frees the target's old handle only");
        expect(a.p == nullptr && a.cap == 0 && b.p == &g_cells[1] && b.cap == 1, "move assignment carries over");
    }
    expect(freed(1) == 1 && freed(2) == 1, "handles 1 and 2 freed once");
    {  // self-move assignment keeps the handle
        Fake a = make(3, 3);
        Fake &same = a;
        a = std::move(same);
        expect(a.p == &g_cells[3] && a.cap == 3 && freed(3) == 0, "self-move keeps the handle");
    }
    expect(freed(3) == 1, "handle 3 freed once");
    {  // reset twice
        Fake a = make(4, 4);
        a.reset();
        expect(a.p == nullptr && a.cap == 0 && freed(4) == 1, "reset frees and empties");
        a.reset();
        expect(freed(4) == 1, "a second reset frees nothing");
    }
    expect(freed(4) == 1, "handle 4 freed once");
    {  // a vector of owners growing (moves) and an empty owner
        std::vector<Fake> v;
        for (int k = 5; k < 12; ++k) v.push_back(make(k, (size_t)k));
        Fake none;
        expect(!none && none.cap == 0, "a default owner is empty");
        for (int k = 5; k < 12; ++k) expect(freed(k) == 0, "growing a vector frees nothing");
    }
    for (int k = 5; k < 12; ++k) expect(freed(k) == 1, "vector elements freed once");
    expect(g_freed.count(nullptr) == 0, "null is never freed");
    for (auto &kv : g_freed) expect(kv.second == 1, "every handle freed exactly once");
    expect(g_freed.size() == 12, "every handle freed");
    // the error mapping (no HIP call: enumerators only)
    expect(tspgpu::hip_err(hipSuccess) == 0 && tspgpu::hip_err(hipErrorOutOfMemory) == -ENOMEM &&
               tspgpu::hip_err(hipErrorNoDevice) == -ENODEV && tspgpu::hip_err(hipErrorInvalidDevice) == -ENODEV &&
               tspgpu::hip_err(hipErrorInvalidValue) == -EIO,
           "hip_err mapping");
    if (g_failures) return 1;
    std::printf("check_hipbuf: ok\n");
    return 0;
}
