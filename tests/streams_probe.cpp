// rocRAND's own host-callable Philox4x32-10 (rocrand_init, rocrand4, rocrand_uniform_double2, rocrand_normal_double2 are
// __device__ __host__) for the (seed, subsequence, offset) triples of the command line, three hexadecimal words each.  One
// line per triple, every field hexadecimal, doubles as their bit patterns:
//   seed subsequence offset  w0 w1 w2 w3  u.x u.y  n.x n.y  c.x c.y
// w = rocrand4, u = rocrand_uniform_double2, n = rocrand_normal_double2, each on a freshly initialised state; c = the
// rocrand_normal_double2 that follows a rocrand_uniform_double2 on one state, as t1d_random_meals draws a candidate.
// Host only, no HIP call.  Built and run by test_streams_host.py, which compares the lines with oracle/t1d_streams.py.
#include <hip/hip_runtime.h>
#include <rocrand/rocrand_kernel.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static unsigned long long bits_of(double v)
{
    unsigned long long b;
    std::memcpy(&b, &v, sizeof(b));
    return b;
}

int main(int argc, char** argv)
{
    if (argc < 4 || (argc - 1) % 3 != 0) {
        std::fprintf(stderr, "usage: %s seed subsequence offset [seed subsequence offset ...]   (hexadecimal)\n", argv[0]);
        return 2;
    }
    for (int a = 1; a + 2 < argc; a += 3) {
        const unsigned long long seed = std::strtoull(argv[a], nullptr, 16), sub = std::strtoull(argv[a + 1], nullptr, 16),
                                 off = std::strtoull(argv[a + 2], nullptr, 16);
        rocrand_state_philox4x32_10 st;
        rocrand_init(seed, sub, off, &st);
        const uint4 w = rocrand4(&st);
        rocrand_init(seed, sub, off, &st);
        const double2 u = rocrand_uniform_double2(&st);
        const double2 c = rocrand_normal_double2(&st);
        rocrand_init(seed, sub, off, &st);
        const double2 n = rocrand_normal_double2(&st);
        std::printf("%llx %llx %llx  %08x %08x %08x %08x  %016llx %016llx  %016llx %016llx  %016llx %016llx\n", seed, sub, off,
                    w.x, w.y, w.z, w.w, bits_of(u.x), bits_of(u.y), bits_of(n.x), bits_of(n.y), bits_of(c.x), bits_of(c.y));
    }
    return 0;
}
