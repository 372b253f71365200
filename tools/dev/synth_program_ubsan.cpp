// Stand-alone sanitizer check of K23's host-compilable side (csrc/sv_synth_host.h: phase A's pixel with all its clamping and clipping,
// the per-pixel bodies of the new ops, the job check, the tap helper).  Host code only; never loaded into Python and never run on a GPU
// machine:
//     c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/dev/synth_program_ubsan.cpp -o synth_program_ubsan && ./synth_program_ubsan
// Runs every refusal of the check, extreme integers and random bytes as records, the tap helper at its edges, and -- from exactly-sized
// heap buffers, so that ASan sees any access outside them -- the very functions the kernel calls over the malformed records of
// tests/test_gpu_synth_cells.py::test_kernel_survives_what_the_check_refuses and over random bytes.  Exits 0 when clean.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../sudoku-vision_amd/csrc/sv_synth_host.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static sv_syn_cell cell(int kind = SV_SYN_BG_PLAIN, int value = 255)
{
    sv_syn_cell c;
    memset(&c, 0, sizeof c);
    c.bg_kind = kind;
    c.bg_value = value;
    c.glyph_slot = -1;
    return c;
}

static sv_aug_step step(int op, std::initializer_list<int> i = {}, std::initializer_list<double> d = {})
{
    sv_aug_step s;
    memset(&s, 0, sizeof s);
    s.op = op;
    int k = 0;
    for (int v : i) s.i[k++] = v;
    k = 0;
    for (double v : d) s.d[k++] = v;
    return s;
}

static int check_one(const sv_syn_cell &c, const std::vector<sv_aug_step> &chain, const char *expect, int size = 28, int n_steps = -1, int slots = 1, int gw = 11, int gh = 18)
{
    std::vector<sv_aug_step> steps(SV_AUG_MAX_STEPS);
    memset(steps.data(), 0, steps.size() * sizeof(sv_aug_step));
    for (size_t k = 0; k < chain.size() && k < steps.size(); k++) steps[k] = chain[k];
    std::vector<sv_syn_cell> cells(1, c);
    std::vector<int32_t> ns(1, n_steps == -1 ? (int)chain.size() : n_steps), dims(2 * (slots > 0 ? slots : 1));
    for (int s = 0; s < slots; s++) { dims[2 * s] = gw; dims[2 * s + 1] = gh; }
    std::vector<char> msg(256);
    const int rc = sv_syn_check_program(cells.data(), steps.data(), ns.data(), 1, size, slots > 0 ? dims.data() : nullptr, slots, msg.data(), msg.size());
    if (expect && !(rc == SV_ERR_BAD_ARG && strstr(msg.data(), expect))) { std::printf("expected \"%s\", got rc %d \"%s\"\n", expect, rc, rc ? msg.data() : ""); fails++; }
    if (!expect && rc != SV_OK) { std::printf("expected SV_OK, got \"%s\"\n", msg.data()); fails++; }
    return rc;
}

// the whole of what a workgroup does with one output, on the host: phase A into an exactly-sized plane, then the new ops' pixel bodies
static void run_output(const sv_syn_cell &c, const std::vector<sv_aug_step> &chain, int size, const std::vector<uint8_t> &atlas, const std::vector<int32_t> &dims, int n_slots,
                       std::vector<uint8_t> &out)
{
    std::vector<uint8_t> a(size * size), b(size * size), prev(size * size, 171);
    for (int y = 0; y < size; y++)
        for (int x = 0; x < size; x++) a[y * size + x] = sv_syn_base_pixel(c, size, x, y, 42, 7, n_slots ? atlas.data() : nullptr, n_slots ? dims.data() : nullptr, n_slots, prev.data());
    for (const sv_aug_step &st : chain) {
        if (st.op == SV_SYN_GAUSS_BLUR && (st.i[0] == 3 || st.i[0] == 5)) {
            for (int y = 0; y < size; y++)
                for (int x = 0; x < size; x++) b[y * size + x] = sv_syn_blur_px(a.data(), size, size, x, y, st.i[0], st.i + 1);
            a.swap(b);
        } else if (st.op == SV_SYN_ERODE || st.op == SV_SYN_DILATE) {
            for (int y = 0; y < size; y++)
                for (int x = 0; x < size; x++) b[y * size + x] = sv_syn_morph_px(a.data(), size, size, x, y, st.op == SV_SYN_DILATE);
            a.swap(b);
        }
    }
    out = a;
}

int main()
{
    static_assert(sizeof(sv_syn_cell) == 96 && alignof(sv_syn_cell) == 8, "sv_syn_cell is 96 bytes, 8-byte aligned");
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int imax = std::numeric_limits<int>::max(), imin = std::numeric_limits<int>::min();

    // well-formed
    check_one(cell(), {step(SV_SYN_AFFINE_CONST, {255}, {1, 0, 2, 0, 1, -1}), step(SV_SYN_PERSPECTIVE_CONST, {0}, {1, 0, 0, 0, 1, 0, 0, 0, 1}), step(SV_SYN_SCALE_PAD, {1, 1, 0, 255}),
                       step(SV_SYN_SCALE_PAD, {34, 34, 1, 255}), step(SV_SYN_GAUSS_BLUR, {5, 102, 62, 15}), step(SV_SYN_ERODE), step(SV_SYN_DILATE), step(SV_AUG_BRIGHTNESS, {}, {-15}),
                       step(SV_AUG_NOISE_GAUSS, {}, {7.65}), step(SV_AUG_BLUR, {3})}, nullptr);
    // every refusal
    { sv_syn_cell c = cell(5); check_one(c, {}, "bg_kind"); c = cell(imin); check_one(c, {}, "bg_kind"); }
    for (int v : {256, -1, imax, imin}) check_one(cell(SV_SYN_BG_PLAIN, v), {}, "bg_value");
    { sv_syn_cell c = cell(SV_SYN_BG_NOISY); c.bg_d[0] = nan; check_one(c, {}, "sigma is not finite"); c.bg_kind = SV_SYN_BG_TEXTURED; c.bg_d[0] = inf; check_one(c, {}, "sigma is not finite"); }
    { sv_syn_cell c = cell(SV_SYN_BG_GRADIENT); c.grad_dir = 3; check_one(c, {}, "grad_dir"); c.grad_dir = imin; check_one(c, {}, "grad_dir"); c.grad_dir = 1; c.bg_d[2] = nan; check_one(c, {}, "gradient term"); }
    for (int v : {1, 5, -2, imax, imin}) { sv_syn_cell c = cell(SV_SYN_BG_TEXTURED); c.grain_stride = v; c.grain_d[0] = c.grain_d[1] = 0x55555555u; check_one(c, {}, "grain_stride"); }
    { sv_syn_cell c = cell(SV_SYN_BG_TEXTURED); c.grain_stride = 2; c.grain_d[0] = 0x55555555u; c.grain_d[1] = 0; check_one(c, {}, "grain_d: row 32", 64); check_one(c, {}, nullptr, 28); }
    for (int v : {16, -1, imax, imin}) { sv_syn_cell c = cell(); c.art_edges = v; c.art_width = 1; check_one(c, {}, "art_edges"); }
    for (int v : {0, 3, imax, imin}) { sv_syn_cell c = cell(); c.art_edges = 5; c.art_width = v; check_one(c, {}, "art_width"); }
    { sv_syn_cell c = cell(); c.art_edges = 5; c.art_width = 2; c.art_dark = 256; check_one(c, {}, "art_dark"); }
    for (auto m : {std::initializer_list<int>{24, 0, 5, 210}, {-1, 0, 2, 210}, {0, 0, 2, 256}, {0, 0, 29, 0}, {imax, imax, imax, 0}, {imin, imin, imin, imin}, {0, 0, -1, 0}}) {
        sv_syn_cell c = cell();
        int k = 0;
        for (int v : m) c.smudge[k++] = v;
        check_one(c, {}, "smudge");
    }
    for (int v : {1, -2, imax, imin}) { sv_syn_cell c = cell(); c.glyph_slot = v; check_one(c, {}, "glyph_slot"); }
    { sv_syn_cell c = cell(); c.glyph_slot = 0; c.glyph_ink = 256; check_one(c, {}, "glyph_ink"); check_one(c, {}, "glyph_slot", 28, -1, 0); }
    check_one(cell(), {}, "atlas slot 0", 28, -1, 1, 33, 10);
    check_one(cell(), {}, "atlas slot 0", 28, -1, 1, 10, 0);
    check_one(cell(), {}, "atlas slot 0", 28, -1, 2, imin, imax);
    check_one(cell(), {}, "steps", 28, 11);
    check_one(cell(), {}, "steps", 28, imin);
    check_one(cell(), {}, "bad shape", 3);
    check_one(cell(), {}, "bad shape", imax);
    for (int op : {38, 31, 11, -1, imax, imin}) check_one(cell(), {step(op)}, "unknown op");
    check_one(cell(), {step(SV_SYN_AFFINE_CONST, {255}, {1, 0, inf, 0, 1, 0})}, "affine matrix is not finite");
    check_one(cell(), {step(SV_SYN_PERSPECTIVE_CONST, {255}, {1, 0, 0, 0, 1, 0, 0, 0, nan})}, "perspective matrix is not finite");
    for (int v : {256, -1, imax, imin}) { check_one(cell(), {step(SV_SYN_AFFINE_CONST, {v}, {1, 0, 0, 0, 1, 0})}, "border value"); check_one(cell(), {step(SV_SYN_PERSPECTIVE_CONST, {v}, {1, 0, 0, 0, 1, 0, 0, 0, 1})}, "border value"); }
    for (auto &s : {step(SV_SYN_SCALE_PAD, {29, 27, 1, 255}), step(SV_SYN_SCALE_PAD, {0, 5, 0, 255}), step(SV_SYN_SCALE_PAD, {57, 57, 1, 255}), step(SV_SYN_SCALE_PAD, {imax, imax, 1, 255}),
                    step(SV_SYN_SCALE_PAD, {imin, imin, 0, 255}), step(SV_SYN_SCALE_PAD, {28, 28, 2, 255})})
        check_one(cell(), {s}, "scale to");
    check_one(cell(), {step(SV_SYN_SCALE_PAD, {20, 20, 0, 300})}, "pad value");
    for (int k : {0, 1, 4, 7, imax, imin}) check_one(cell(), {step(SV_SYN_GAUSS_BLUR, {k, 256, 0, 0})}, "blur kernel");
    for (auto &s : {step(SV_SYN_GAUSS_BLUR, {5, 100, 62, 15}), step(SV_SYN_GAUSS_BLUR, {3, 258, -1, 0}), step(SV_SYN_GAUSS_BLUR, {3, 102, 62, 15}), step(SV_SYN_GAUSS_BLUR, {5, imax, imax, imax}),
                    step(SV_SYN_GAUSS_BLUR, {5, imin, imin, imin}), step(SV_SYN_GAUSS_BLUR, {5, 256, 256, -256})})
        check_one(cell(), {s}, "blur taps");
    check_one(cell(), {step(SV_AUG_CONTRAST, {}, {nan})}, "parameter is not finite");
    check_one(cell(), {step(SV_AUG_BLUR, {4})}, "blur kernel 4");
    check_one(cell(), {step(SV_AUG_FILL_RECT, {imax, imax, imax, imax, imax})}, "rectangle");
    {
        std::vector<char> msg(8);                              // a message buffer shorter than the message
        sv_syn_cell c = cell(SV_SYN_BG_PLAIN, imax);
        sv_aug_step s = step(0);
        int32_t ns = 0;
        CHECK(sv_syn_check_program(&c, &s, &ns, 1, 28, nullptr, 0, msg.data(), msg.size()) == SV_ERR_BAD_ARG && strlen(msg.data()) == 7);
        CHECK(sv_syn_check_program(nullptr, &s, &ns, 1, 28, nullptr, 0, msg.data(), msg.size()) == SV_ERR_BAD_ARG);
        CHECK(sv_syn_check_program(&c, &s, &ns, 0, 28, nullptr, 0, msg.data(), msg.size()) == SV_ERR_BAD_ARG);
        CHECK(sv_syn_check_program(&c, &s, &ns, 1, 28, nullptr, 1, msg.data(), msg.size()) == SV_ERR_BAD_ARG);
    }

    // the tap helper
    int32_t t[3];
    for (int k : {3, 5})
        for (double sigma : {0.3, 0.5, 1.0, 2.5, 1e-300, 1e-3, 1e3, 1e300}) {
            CHECK(sv_syn_gaussian_taps_q8(k, sigma, t));
            CHECK(t[0] + 2 * t[1] + 2 * t[2] == 256 && t[0] >= 0 && t[1] >= 0 && t[2] >= 0 && (k == 5 || t[2] == 0));
        }
    CHECK(sv_syn_gaussian_taps_q8(3, 0.3, t) && t[0] == 254 && t[1] == 1);
    for (double sigma : {0.0, -1.0, nan, inf, -inf}) CHECK(!sv_syn_gaussian_taps_q8(3, sigma, t));
    for (int k : {0, 1, 4, 7, imax, imin}) CHECK(!sv_syn_gaussian_taps_q8(k, 1.0, t));

    // the records of the GPU robustness test, through the functions the kernel calls: an atlas of one 11 x 18 slot, dims that lie
    {
        const int n_slots = 2;
        std::vector<uint8_t> atlas(n_slots * SV_SYN_GLYPH_SIDE * SV_SYN_GLYPH_SIDE, 200), out;
        std::vector<int32_t> dims = {11, 18, 1000000, -5};      // slot 1 claims a mask larger than the slot and a negative height
        sv_syn_cell bad_slot = cell(SV_SYN_BG_PLAIN, 250);
        bad_slot.glyph_slot = 7;
        run_output(bad_slot, {step(99)}, 28, atlas, dims, n_slots, out);
        for (uint8_t v : out) CHECK(v == 250);
        sv_syn_cell huge = cell(SV_SYN_BG_PLAIN, 1000);          // value above 255, offsets and rectangles at the integer limits
        huge.glyph_slot = 0; huge.glyph_x = imin; huge.glyph_y = imax; huge.glyph_ink = imin;
        huge.smudge[0] = imin; huge.smudge[1] = imin; huge.smudge[2] = imax; huge.smudge[3] = imin;
        huge.art_edges = imax; huge.art_width = imax; huge.art_dark = imax;
        run_output(huge, {step(SV_SYN_GAUSS_BLUR, {5, imax, imin, imax}), step(SV_SYN_GAUSS_BLUR, {9, 1, 1, 1})}, 28, atlas, dims, n_slots, out);
        sv_syn_cell lying = cell(SV_SYN_BG_TEXTURED, -7);
        lying.glyph_slot = 1; lying.glyph_x = -3; lying.glyph_y = -3; lying.glyph_ink = 30; lying.grain_stride = imax; lying.bg_d[0] = nan; lying.grad_dir = imin;
        run_output(lying, {step(SV_SYN_ERODE), step(SV_SYN_DILATE)}, 28, atlas, dims, n_slots, out);
        sv_syn_cell grain = cell(SV_SYN_BG_TEXTURED, 240);
        grain.grain_stride = 2; grain.grain_d[0] = grain.grain_d[1] = ~0u; grain.bg_d[0] = inf; grain.bg_salt = imin;
        for (int size : {4, 12, 28, 63, 64}) run_output(grain, {}, size, atlas, dims, n_slots, out);
        sv_syn_cell grad = cell(SV_SYN_BG_GRADIENT, 245);
        for (int dir : {0, 1, 2}) { grad.grad_dir = dir; grad.bg_d[0] = 1e308; grad.bg_d[1] = -1e308; grad.bg_d[2] = nan; run_output(grad, {}, 64, atlas, dims, n_slots, out); }
        sv_syn_cell keep = cell(SV_SYN_BG_KEEP);
        run_output(keep, {}, 64, atlas, dims, 0, out);
        for (uint8_t v : out) CHECK(v == 171);
    }
    // random bytes as cell records: any image, no fault
    {
        const int n_slots = 3;
        std::vector<uint8_t> atlas(n_slots * SV_SYN_GLYPH_SIDE * SV_SYN_GLYPH_SIDE, 99), out;
        std::vector<int32_t> dims(2 * n_slots);
        for (int round = 0; round < 300; round++) {
            sv_syn_cell c;
            uint32_t *w = (uint32_t *)&c;
            for (int k = 0; k < 24; k += 4) { const sv_philox4 r = sv_philox4x32_10((uint32_t)k, (uint32_t)round, 0, 0, 3, 4); memcpy(w + k, r.v, 16); }
            const sv_philox4 r = sv_philox4x32_10(99, (uint32_t)round, 0, 0, 3, 4);
            for (int k = 0; k < 2 * n_slots; k++) dims[k] = (int32_t)(r.v[k & 3] >> (k & 1 ? 3 : 26)) - 8;
            if (round & 1) { c.bg_kind = (int)(r.v[0] % 5); c.glyph_slot = (int)(r.v[1] % 4); c.glyph_x = (int)(r.v[2] % 40) - 10; c.glyph_y = (int)(r.v[3] % 40) - 10; }
            sv_aug_step s = step(SV_SYN_GAUSS_BLUR, {round & 2 ? 3 : 5, (int)r.v[0], (int)r.v[1], (int)r.v[2]});
            run_output(c, {s, step(SV_SYN_ERODE)}, 4 + round % 61, atlas, dims, n_slots, out);
        }
    }
    std::printf(fails ? "%d checks FAILED\n" : "synth_program_ubsan: clean\n", fails);
    return fails ? 1 : 0;
}
