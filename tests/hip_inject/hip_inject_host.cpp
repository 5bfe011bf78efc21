// The door in front of every checked HIP call (sponge_amd/csrc/pmx_hooks.cpp: pmx::hip_inject), as a program of its own: built twice by
// tests/test_hip_inject_host.py under -fsanitize=address,undefined - with -DPMX_TEST_HOOKS (the counting, arming variant of the test
// library) and without (the shipped variant) - and run directly.  No HIP call is made: the few symbols of the library that pmx_hooks.cpp
// refers to are stubs here.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "pmx_hooks.cpp"

namespace pmx {
static char g_text[512] = "";
int set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_text, sizeof g_text, fmt, ap);
    va_end(ap);
    return code;
}
int hip_fail(hipError_t, const char *what) { return set_error(PMX_ERR_HIP, "%s", what); }
hipError_t launch_hash_strided(const DevConfig &, uint32_t, const uint64_t *, size_t, size_t, size_t, uint64_t *, size_t, size_t, hipStream_t) {
    return hipSuccess;
}
}  // namespace pmx

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

// what PMX_HIP does with a call: the number of times `made` was incremented says whether the call itself ran
static hipError_t checked(int &made) { return PMX_HIP_CALL((++made, hipSuccess)); }

int main() {
    int made = 0;
#ifdef PMX_TEST_HOOKS
    // disarmed: everything passes and is counted
    CHECK(pmx_test_fail_hip(0) == PMX_OK && pmx_test_hip_calls() == 0);
    for (int i = 0; i < 5; ++i) CHECK(checked(made) == hipSuccess);
    CHECK(made == 5 && pmx_test_hip_calls() == 5 && pmx::hip_injected() == nullptr && pmx_test_hip_fired()[0] == 0);
    // armed on the third call from now: 1 and 2 pass, 3 fails and is not made, 4 and 5 pass again (one shot)
    CHECK(pmx_test_fail_hip(3) == PMX_OK && pmx_test_hip_calls() == 0);
    made = 0;
    CHECK(checked(made) == hipSuccess && checked(made) == hipSuccess && made == 2 && pmx::hip_injected() == nullptr);
    CHECK(checked(made) == hipErrorOutOfMemory && made == 2 && pmx_test_hip_calls() == 3);
    const char *note = pmx::hip_injected();
    CHECK(note && strstr(note, "injected") && strstr(note, "++made"));       // the word and the expression text
    CHECK(pmx::hip_injected() == nullptr);                                    // asked once
    CHECK(strstr(pmx_test_hip_fired(), "injected") != nullptr);               // the hook keeps it until the next arm
    CHECK(checked(made) == hipSuccess && checked(made) == hipSuccess && made == 4 && pmx_test_hip_calls() == 5);
    // the wording outlives the checked calls of an unwinding, and is gone once a site that absorbed the failure has asked, or with the next arm
    CHECK(pmx_test_fail_hip(1) == PMX_OK);
    CHECK(checked(made) == hipErrorOutOfMemory && checked(made) == hipSuccess && pmx::hip_injected() != nullptr && pmx::hip_injected() == nullptr);
    CHECK(pmx_test_fail_hip(1) == PMX_OK && checked(made) == hipErrorOutOfMemory && pmx_test_fail_hip(0) == PMX_OK && pmx::hip_injected() == nullptr);
    // the first call, and a count no call reaches
    CHECK(pmx_test_fail_hip(1) == PMX_OK);
    made = 0;
    CHECK(checked(made) == hipErrorOutOfMemory && made == 0 && pmx::hip_injected() != nullptr);
    CHECK(pmx_test_fail_hip((int64_t)1 << 40) == PMX_OK);
    for (int i = 0; i < 1000; ++i) CHECK(checked(made) == hipSuccess);
    CHECK(made == 1000 && pmx_test_hip_calls() == 1000 && pmx_test_hip_fired()[0] == 0);
    CHECK(pmx_test_fail_hip(-1) == PMX_ERR_ARG);
    // per thread: this thread is armed on its next call; a second thread makes calls meanwhile - none fails, none is counted here,
    // and its own count starts at 0
    CHECK(pmx_test_fail_hip(1) == PMX_OK);
    int other_made = 0, other_failed = 0;
    int64_t other_before = -1, other_after = -1;
    std::thread other([&] {
        other_before = pmx_test_hip_calls();
        for (int i = 0; i < 7; ++i) other_failed += checked(other_made) != hipSuccess;
        other_after = pmx_test_hip_calls();
    });
    other.join();
    CHECK(other_made == 7 && other_failed == 0 && other_before == 0 && other_after == 7);
    CHECK(pmx_test_hip_calls() == 0);
    made = 0;
    CHECK(checked(made) == hipErrorOutOfMemory && made == 0);
    // the pool view refuses null pointers before it touches anything
    size_t a = 0, b = 0, c = 0;
    CHECK(pmx_test_pass_pool(nullptr, &a, &b, &c) == PMX_ERR_ARG);
    {
        pmx_ctx ctx;
        ctx.pass_pool.resize(3);
        ctx.pass_pool[0].recorded = true;
        ctx.pass_pool[1].recorded = ctx.pass_pool[1].poisoned = true;
        CHECK(pmx_test_pass_pool(&ctx, &a, &b, &c) == PMX_OK && a == 3 && b == 1 && c == 1);
    }
    CHECK(pmx_test_fail_hip(0) == PMX_OK);
    puts("test variant ok");
#else
    // the shipped variant: a constant, whatever is asked and however often
    for (int i = 0; i < 1000; ++i) CHECK(checked(made) == hipSuccess);
    CHECK(made == 1000 && pmx::hip_injected() == nullptr);
    std::thread other([&] { CHECK(pmx::hip_inject("x") == hipSuccess && pmx::hip_injected() == nullptr); });
    other.join();
    puts("shipped variant ok");
#endif
    return 0;
}
