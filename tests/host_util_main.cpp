// Stand-alone check of articulatory_amd/csrc/hificar_host_util.h (tests/test_host_util.py builds it with the host compiler under
// -fsanitize=address,undefined and runs it): Carver, WeightIntake, TapTable and check_workspace, with a stub for the library's fail().
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static char g_err[1024] = "";
static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#include "hificar_host_util.h"

static int g_failed = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                          \
        }                                                                        \
    } while (0)

static bool said(const char* text) { return strstr(g_err, text) != nullptr; }

static size_t round_up(size_t x, size_t m) { return (x + m - 1) / m * m; }

// one carve of `sizes` (the buffer at index `skip` is conditional and not taken): every pointer, and the total
static size_t carve(void* base, size_t granule, const std::vector<size_t>& sizes, int skip, std::vector<char*>* out) {
    Carver cv(base, granule);
    for (size_t i = 0; i < sizes.size(); ++i) out->push_back((int)i == skip ? nullptr : cv.take<char>(sizes[i]));
    return cv.bytes();
}

static void test_carver() {
    const std::vector<size_t> sizes = {1, 255, 256, 257, 0, 1000, 1024, 1025, 4, 3 * 1024};
    for (size_t granule : {(size_t)256, (size_t)1024}) {
        std::vector<char*> none, real;
        const size_t total = carve(nullptr, granule, sizes, -1, &none);
        size_t want = 0;
        for (size_t s : sizes) want += round_up(s, granule);
        CHECK(total == want);
        for (char* p : none) CHECK(p == nullptr);
        void* mem = nullptr;
        CHECK(posix_memalign(&mem, 1024, total) == 0);  // (exactly `total` bytes: a write past them is the sanitizer's to report)
        char* base = static_cast<char*>(mem);
        CHECK(carve(base, granule, sizes, -1, &real) == total);  // a null base and a real base: the same total
        for (size_t i = 0; i < sizes.size(); ++i) {
            CHECK((size_t)(real[i] - base) % granule == 0);
            memset(real[i], (int)i + 1, sizes[i]);  // (in bounds of the `total` bytes: the sanitizer's to judge)
            if (i + 1 < sizes.size()) {
                CHECK(real[i + 1] >= real[i] + sizes[i]);                                     // increasing, and no overlap by the sizes asked
                CHECK(sizes[i] != 0 || real[i + 1] == real[i]);                               // a zero-byte take advances nothing
            } else CHECK(real[i] + sizes[i] <= base + total);
        }
        for (size_t i = 0; i < sizes.size(); ++i)
            for (size_t b = 0; b < sizes[i]; ++b) CHECK(real[i][b] == (char)(i + 1));  // nobody's bytes were written twice
        // a conditional buffer that is not taken stays null and costs nothing: the others lie where they lie in a carve without it
        std::vector<char*> skipped, without;
        std::vector<size_t> fewer = sizes;
        fewer.erase(fewer.begin() + 3);
        const size_t t_skipped = carve(base, granule, sizes, 3, &skipped), t_without = carve(base, granule, fewer, -1, &without);
        CHECK(t_skipped == t_without && t_skipped == total - round_up(sizes[3], granule));
        CHECK(skipped[3] == nullptr);
        skipped.erase(skipped.begin() + 3);
        CHECK(skipped == without);
        // the offset form agrees with the pointer form
        Carver by_ptr(base, granule), by_off(nullptr, granule);
        for (size_t elems : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)0, (size_t)300}) {
            float* p = by_ptr.floats(elems);
            const size_t at = by_off.floats_at(elems);
            CHECK(reinterpret_cast<char*>(p) == base + at * sizeof(float));
            CHECK(by_ptr.bytes() == by_off.bytes());
        }
        Carver bytes_form(base, granule);
        CHECK(bytes_form.take_at(5) == 0 && bytes_form.take_at(5) == granule && bytes_form.take<int>(0) == reinterpret_cast<int*>(base + 2 * granule));
        free(base);
    }
}

static void test_weight_intake() {
    WeightIntake w;
    w.expected["b"] = {4};
    w.expected["a"] = {2, 3};
    w.expected["B"] = {1};  // (the map's order: "B" < "a" < "b")
    const float six[6] = {1, 2, 3, 4, 5, 6}, other[6] = {9, 8, 7, 6, 5, 4};
    const int64_t s23[2] = {2, 3}, s32[2] = {3, 2}, s4[1] = {4}, s1[1] = {1};
    CHECK(w.first_missing() && *w.first_missing() == "B");
    CHECK(w.check_complete() == HIFICAR_E_STATE && said("Missing key(s) in state_dict: \"B\""));
    CHECK(w.set("zz", six, s23, 2) == HIFICAR_E_INVALID && said("unexpected tensor name 'zz' for this configuration"));
    CHECK(w.tensors.empty());
    CHECK(w.set("a", six, s32, 2) == HIFICAR_E_INVALID && said("size mismatch for a: expected (2,3,) got (3,2,)"));
    CHECK(w.set("a", six, s23, 1) == HIFICAR_E_INVALID && said("size mismatch for a: expected (2,3,) got (2,)"));
    CHECK(w.tensors.empty());  // the refusals leave the staged set unchanged
    CHECK(w.set("a", six, s23, 2) == HIFICAR_OK && w.tensors.size() == 1 && w.data("a") == std::vector<float>(six, six + 6));
    CHECK(w.at("a").shape == std::vector<int64_t>({2, 3}));
    CHECK(w.set("zz", six, s23, 2) == HIFICAR_E_INVALID && w.tensors.size() == 1 && w.data("a")[0] == 1.f);
    CHECK(w.set("a", other, s23, 2) == HIFICAR_OK && w.tensors.size() == 1 && w.data("a") == std::vector<float>(other, other + 6));  // replaced
    CHECK(*w.first_missing() == "B");
    CHECK(w.set("B", six, s1, 1) == HIFICAR_OK && *w.first_missing() == "b");
    CHECK(w.set("b", six, s4, 1) == HIFICAR_OK && w.first_missing() == nullptr && w.check_complete() == HIFICAR_OK);
    w.clear_staged();
    CHECK(w.tensors.empty() && w.expected.size() == 3 && w.expected.at("a") == std::vector<int64_t>({2, 3}));  // expected survives
    CHECK(*w.first_missing() == "B");
}

static void test_tap_table() {
    TapTable t;
    float buf[8], other[4];
    float* dst = buf;
    CHECK(t.empty() && !t.wanted("x"));
    CHECK(t.find("x", 100, &dst) == HIFICAR_OK && dst == nullptr);  // not tapped: nothing to copy, nothing refused
    t.set("x", buf, 8);
    t.set("layers.0.convs1.1", other, 4);
    CHECK(!t.empty() && t.wanted("x") && t.wanted("layers.0.convs1.1") && !t.wanted("y"));
    CHECK(t.any_contains(".convs1.") && !t.any_contains(".convs2."));
    CHECK(t.find("x", 8, &dst) == HIFICAR_OK && dst == buf);  // exact capacity passes
    CHECK(t.find("x", 9, &dst) == HIFICAR_E_INVALID && dst == nullptr && said("debug tap 'x' needs 9 floats, buffer has 8"));  // one float short
    t.set("x", other, 4);  // a second set replaces the first
    CHECK(t.find("x", 4, &dst) == HIFICAR_OK && dst == other);
    t.set("x", nullptr, 0);  // forget one
    CHECK(!t.wanted("x") && t.wanted("layers.0.convs1.1"));
    t.set("never set", nullptr, 0);
    CHECK(!t.empty());
    t.set(nullptr, buf, 8);  // forget all
    CHECK(t.empty() && !t.wanted("layers.0.convs1.1"));
}

static void test_check_workspace() {
    alignas(256) static char ws[512];
    CHECK(check_workspace(nullptr, nullptr, 512, 1) == HIFICAR_E_INVALID && strcmp(g_err, "workspace must be a 256-byte aligned device pointer") == 0);
    CHECK(check_workspace(nullptr, ws + 4, 512, 1) == HIFICAR_E_INVALID);
    CHECK(check_workspace(nullptr, ws, 10, 20) == HIFICAR_E_WORKSPACE && strcmp(g_err, "workspace too small: 10 < 20") == 0);
    CHECK(check_workspace("f", ws, 10, 20) == HIFICAR_E_WORKSPACE && strcmp(g_err, "f: workspace too small: 10 < 20") == 0);
    CHECK(check_workspace("f", ws + 256, 20, 20) == HIFICAR_OK);
    CHECK(check_workspace(nullptr, ws + 4, 0, 20) == HIFICAR_E_INVALID);  // the alignment is refused first
}

int main() {
    test_carver();
    test_weight_intake();
    test_tap_table();
    test_check_workspace();
    if (g_failed) {
        fprintf(stderr, "%d check(s) failed\n", g_failed);
        return 1;
    }
    printf("host_util: ok\n");
    return 0;
}
