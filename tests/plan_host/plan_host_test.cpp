// The launch-plan recorder (patchmatchnet_amd/csrc/plan.hip) as a plain host program: appending, the fork/join bookkeeping, replay
// order by part and destroy, over host stubs for the HIP calls (hip_stubs.hpp).  Built with -fsanitize=address,undefined and run on
// the CPU by tests/test_plan_host.py; exit status 0 = every check held and the sanitizers saw nothing.
#include <cstdio>
#include <cstdlib>
#include <string>

#define PMN_PLAN_HOST_STUBS "../../tests/plan_host/hip_stubs.hpp"
#include "../../patchmatchnet_amd/csrc/plan.hip"

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static void kernel_a() {}
static void kernel_b() {}

// what PMN_LAUNCH does while the thread records: one long long and one odd-sized struct (alignment padding inside the blob)
struct Odd {
    char c[3];
};
static void record(const void* func, long long tag) {
    Odd odd{{1, 2, 3}};
    double d = 0.5;
    void* args[] = {&tag, &odd, &d};
    const size_t sizes[] = {sizeof tag, sizeof odd, sizeof d}, aligns[] = {alignof(long long), alignof(Odd), alignof(double)};
    CHECK(pmn_tls_plan != nullptr);
    CHECK(pmn_plan_append(pmn_tls_plan, func, dim3((unsigned)tag), dim3(64), 0, 3, args, sizes, aligns) == PMN_OK);
}

static void* fresh() {
    void* p = nullptr;
    CHECK(pmn_plan_create(&p) == PMN_OK && p);
    return p;
}

int main() {
    const void* A = reinterpret_cast<const void*>(&kernel_a);
    const void* B = reinterpret_cast<const void*>(&kernel_b);
    int main_stream = 0, side_stream = 0;
    void* S = &main_stream;
    void* T = &side_stream;

    // ---- error paths of the markers --------------------------------------------------------------------------------------------
    void* p = fresh();
    CHECK(pmn_plan_fork(p) == PMN_ERR_ARG && pmn_plan_join(p) == PMN_ERR_ARG && pmn_plan_switch(p, 1) == PMN_ERR_ARG);  // not recording
    CHECK(pmn_plan_begin(p) == PMN_OK);
    CHECK(pmn_plan_join(p) == PMN_ERR_ARG);       // join without a fork
    CHECK(pmn_plan_switch(p, 1) == PMN_ERR_ARG);  // switch outside a fork
    CHECK(pmn_plan_fork(p) == PMN_OK);
    CHECK(pmn_plan_fork(p) == PMN_ERR_ARG);  // nested
    CHECK(pmn_plan_switch(p, 2) == PMN_ERR_ARG && pmn_plan_switch(p, -1) == PMN_ERR_ARG);
    CHECK(pmn_plan_end(p) == PMN_ERR_ARG);  // open fork
    CHECK(pmn_plan_launch(p, S) == PMN_ERR_ARG && pmn_plan_launch_part(p, 0, S) == PMN_ERR_ARG);
    CHECK(pmn_tls_plan == nullptr);
    CHECK(pmn_plan_destroy(p) == PMN_OK);

    p = fresh();
    CHECK(pmn_plan_begin(p) == PMN_OK && pmn_plan_fork(p) == PMN_OK && pmn_plan_join(p) == PMN_OK);
    CHECK(pmn_plan_fork(p) == PMN_ERR_ARG && pmn_plan_switch(p, 0) == PMN_ERR_ARG && pmn_plan_join(p) == PMN_ERR_ARG);  // one region
    CHECK(pmn_plan_end(p) == PMN_OK && pmn_plan_count(p) == 2);
    CHECK(pmn_plan_fork(p) == PMN_ERR_ARG);  // sealed
    CHECK(pmn_plan_destroy(p) == PMN_OK);

    // ---- a forward's shape: two launches, fork, side / main interleaved, join, one launch ------------------------------------------
    p = fresh();
    CHECK(pmn_plan_begin(p) == PMN_OK);
    record(A, 1);
    record(B, 2);
    CHECK(pmn_plan_fork(p) == PMN_OK);
    record(A, 3);  // main until switched
    CHECK(pmn_plan_switch(p, 1) == PMN_OK);
    record(B, 4);
    record(B, 5);
    CHECK(pmn_plan_switch(p, 0) == PMN_OK);
    record(A, 6);
    CHECK(pmn_plan_switch(p, 1) == PMN_OK);
    record(B, 7);
    CHECK(pmn_plan_join(p) == PMN_OK);
    record(A, 8);
    for (int i = 0; i < 200; ++i) record(B, 100 + i);  // (the blob and the entry list grow past their first allocations)
    CHECK(pmn_plan_end(p) == PMN_OK);
    CHECK(pmn_plan_count(p) == 8 + 2 + 200);
    const int want_branch[] = {0, 0, 0, 0, 1, 1, 0, 1, 0, 0};
    for (int i = 0; i < 10; ++i) CHECK(pmn_plan_entry_branch(p, i) == want_branch[i]);
    CHECK(pmn_plan_entry_branch(p, -1) == PMN_ERR_ARG && pmn_plan_entry_branch(p, 210) == PMN_ERR_ARG);
    CHECK(std::string(pmn_plan_kernel_name(p, 2)) == "<fork>" && std::string(pmn_plan_kernel_name(p, 8)) == "<join>");
    CHECK(std::string(pmn_plan_kernel_name(p, 0)) == "stub_kernel" && pmn_plan_kernel_name(p, 210) == nullptr);

    // the whole plan on one stream: recorded order
    CHECK(pmn_plan_launch(p, S) == PMN_OK && stub_launches.size() == 208);
    const long long order[] = {1, 2, 3, 4, 5, 6, 7, 8, 100};
    for (int i = 0; i < 9; ++i) CHECK(stub_launches[i].arg0 == order[i] && stub_launches[i].stream == S);
    CHECK(stub_launches[0].func == A && stub_launches[1].func == B && stub_launches[0].grid_x == 1 && stub_launches[207].arg0 == 299);
    stub_launches.clear();

    // by part: the sequence include/pmn_hip.h gives
    CHECK(pmn_plan_launch_part(p, PMN_PLAN_PART_PRE, S) == PMN_OK && stub_launches.size() == 2);
    CHECK(pmn_plan_launch_part(p, PMN_PLAN_PART_SIDE, T) == PMN_OK && stub_launches.size() == 5);
    CHECK(pmn_plan_launch_part(p, PMN_PLAN_PART_MAIN, S) == PMN_OK && stub_launches.size() == 7);
    CHECK(pmn_plan_launch_part(p, PMN_PLAN_PART_POST, S) == PMN_OK && stub_launches.size() == 208);
    const long long by_part[] = {1, 2, 4, 5, 7, 3, 6, 8};
    for (int i = 0; i < 8; ++i) {
        CHECK(stub_launches[i].arg0 == by_part[i]);
        CHECK(stub_launches[i].stream == ((i >= 2 && i < 5) ? T : S));
    }
    CHECK(pmn_plan_launch_part(p, 4, S) == PMN_ERR_ARG && pmn_plan_launch_part(p, -1, S) == PMN_ERR_ARG);
    stub_launches.clear();
    stub_fail_launch = true;
    CHECK(pmn_plan_launch(p, S) == PMN_ERR_LAUNCH && pmn_plan_launch_part(p, PMN_PLAN_PART_SIDE, T) == PMN_ERR_LAUNCH);
    stub_fail_launch = false;
    CHECK(pmn_plan_destroy(p) == PMN_OK);

    // ---- a plan without a region is all "before the fork" ------------------------------------------------------------------------------
    p = fresh();
    CHECK(pmn_plan_begin(p) == PMN_OK);
    record(A, 1);
    record(B, 2);
    CHECK(pmn_plan_end(p) == PMN_OK);
    CHECK(pmn_plan_launch_part(p, PMN_PLAN_PART_SIDE, T) == PMN_OK && pmn_plan_launch_part(p, PMN_PLAN_PART_MAIN, S) == PMN_OK &&
          pmn_plan_launch_part(p, PMN_PLAN_PART_POST, S) == PMN_OK && stub_launches.empty());
    CHECK(pmn_plan_launch_part(p, PMN_PLAN_PART_PRE, S) == PMN_OK && stub_launches.size() == 2);
    CHECK(pmn_plan_entry_branch(p, 0) == 0 && pmn_plan_entry_branch(p, 1) == 0);
    CHECK(pmn_plan_destroy(p) == PMN_OK);

    // ---- destroy while recording releases the thread ---------------------------------------------------------------------------------
    p = fresh();
    CHECK(pmn_plan_begin(p) == PMN_OK && pmn_plan_fork(p) == PMN_OK);
    record(A, 1);
    CHECK(pmn_plan_destroy(p) == PMN_OK && pmn_tls_plan == nullptr);
    p = fresh();
    CHECK(pmn_plan_begin(p) == PMN_OK && pmn_plan_end(p) == PMN_OK && pmn_plan_count(p) == 0 && pmn_plan_destroy(p) == PMN_OK);
    std::puts("plan_host_test ok");
    return 0;
}
