"""The launch choice of the coarse-octave strip kernels (csrc/vslam_octave_launch.h) without a GPU: which
k_gauss_h_strip<SH, RI> instantiation or which k_gauss_h_diff row-pair count runs an octave of (rows, cols, nf), over how
many workgroups k_gauss_v_strip splits the levels, on which grids and with how much LDS.  Only this host arithmetic keeps the
items of a workgroup below what an instantiation computes (an item beyond it is silently dropped), so it is swept here over
every width up to past the strip kernels' limit; values of the parent's code are pinned; and the case table of
tests/test_gpu_strip_variants.py is checked against it, so that the GPU cases keep running the variants they are named for.
tests/octave_launch_driver.cpp is the host program, built with the library's vslam_params.cpp for octave sizes and widths."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visualslam_amd", "csrc")

TILE, GENERIC = ("tile",), ("generic",)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("octave_launch")
    exe, obj = d / "driver", d / "vslam_params.o"
    inc = ["-I", CSRC, "-I", os.path.join(ROOT, "include")]
    r = subprocess.run([cxx, "-std=c++17", "-O1", *inc, "-c", os.path.join(CSRC, "vslam_params.cpp"), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *inc, os.path.join(ROOT, "tests", "octave_launch_driver.cpp"), str(obj),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(*args):
        out = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        return out.stdout

    return run


def plans(driver, batches, hdiff=1):
    """[(nf, rows, cols, n_octaves, sigma0)] -> per batch, per octave, the driver's fields as a dict of strings."""
    args = []
    for nf, rows, cols, n_oct, sigma0 in batches:
        args += [nf, rows, cols, n_oct, repr(float(sigma0)), hdiff]
    res = []
    for line in driver("plan", *args).splitlines():
        head, *kv = line.split()
        if head == "case":
            res.append([])
        else:
            res[-1].append(dict(x.split("=", 1) for x in kv))
    assert len(res) == len(batches)
    return res


def tile_widths(driver):
    """Kernel widths of the two k_pyr_octave configurations: the default pyramid's octaves 0 and 1."""
    d = plans(driver, [(1, 64, 64, 2, 1.6)])[0]
    return {d[0]["ke"], d[1]["ke"]}


def variant(oct_fields, tiles):
    """The kernel family and launch variant of one octave, in the notation of tests/test_gpu_strip_variants.py."""
    f = oct_fields
    if f["ke"] in tiles:
        return TILE
    if f["sh"] == "0":
        return GENERIC
    if f["diff"] == "1":
        return ("diff", int(f["npairs"]), int(f["split"]))
    return ("dot2", int(f["SH"]), int(f["RI"]), int(f["split"]))


def test_the_launch_header_needs_no_hip():
    src = open(os.path.join(CSRC, "vslam_octave_launch.h")).read()
    assert "#include <hip" not in src and "__global__" not in src and "hipStream_t" not in src
    # ... and states the choice once: the HIP translation unit has none of its own left
    hip = open(os.path.join(CSRC, "vslam_hip.hip")).read()
    assert "strip_launch(" in hip and "pyr_tile_wide(" in hip and "strip_plan_sh(" in hip
    for gone in ("sh >>= 1", "waste(", "256 / ncs", "want >= 6", "cols <= 1024 ? 16"):
        assert gone not in hip, gone


def test_sweep_every_plan_fits_its_kernel(driver):
    # cols 1..4200 x rows {1..70, 135, 270, 540, 1080, 2160, 2400} x 13 batch sizes x both forms (dot2 at four kernel widths,
    # the difference form with both of its geometries); the driver checks, per plan: dot2 - an instantiated (SH, RI),
    # ceil(cols/8) * (SH/RI) <= strip_item_capacity(RI), LDS <= the limit, grid.y * SH >= rows; difference form - 1 <= npairs <= 8,
    # npairs * ceil(cols/16) <= 256, LDS <= the limit, grid.y * 2 * npairs >= rows; the level split one of 1, 2, 3, 6; no plan
    # beyond 4096 columns.  `first` names the first violated check and its inputs.
    head, *kv = driver("sweep").split()
    got = dict(x.split("=", 1) for x in kv)
    assert head == "sweep" and got["bad"] == "0", got["first"]
    assert int(got["checked"]) == 4200 * 76 * 13 * 6 and int(got["plans"]) > 20_000_000
    # everything that exists is reachable, and nothing else is
    assert got["pairs"] == "4/1,4/4,8/4,16/1,16/2,16/4,"
    assert got["splits"] == "1,2,3,6," and got["npairs"] == "1,2,3,4,5,6,7,8,"


def test_widest_cols_per_rows_per_item(driver):
    # 16 rows per strip, dot2 form: 480 columns are 960 items of one row, 960 columns 960 items of two rows
    assert driver("widest").split() == ["widest", "ri1=480", "ri2=960", "ri4=1024"]


OTHER = "other"  # stands for a base sigma whose octaves match neither a tile configuration nor the difference form's taps

# (nf, frame rows, frame cols, octaves, sigma0) -> {octave: (octave rows, octave cols, variant[, items == capacity])}:
# values of the code before the choice moved into the header
PINS = [
    ((256, 1080, 1920, 4, 1.6), {2: (540, 960, ("diff", 4, 1)), 3: (270, 480, ("diff", 8, 1))}),
    ((128, 16, 512, 2, OTHER), {0: (32, 1024, ("dot2", 16, 4, 1), 512), 1: (16, 512, ("dot2", 8, 4, 1))}),
    ((128, 13, 251, 2, OTHER), {0: (26, 502, ("dot2", 16, 4, 1)), 1: (13, 251, ("dot2", 8, 4, 1))}),
    ((128, 16, 480, 2, OTHER), {0: (32, 960, ("dot2", 16, 2, 1))}),
    ((128, 16, 240, 2, OTHER), {0: (32, 480, ("dot2", 16, 1, 1))}),
    ((128, 8, 1024, 2, OTHER), {0: (16, 2048, ("dot2", 8, 4, 1), 512), 1: (8, 1024, ("dot2", 4, 4, 1))}),
    ((128, 4, 2048, 2, OTHER), {0: (8, 4096, ("dot2", 4, 4, 1), 512)}),
    ((128, 4, 2050, 2, OTHER), {0: (8, 4100, GENERIC), 1: (4, 2050, ("dot2", 4, 4, 1))}),
    ((256, 64, 64, 6, 1.6), {4: (8, 8, ("dot2", 16, 1, 1)), 5: (4, 4, ("dot2", 16, 1, 1))}),
    ((128, 128, 256, 6, 1.6), {4: (16, 32, ("dot2", 8, 4, 2)), 5: (8, 16, ("dot2", 4, 4, 2))}),
]


@pytest.mark.parametrize("sigma_other", [1.2, 2.0])
def test_pinned_choices(driver, sigma_other):
    tiles = tile_widths(driver)
    batches = [(nf, r, c, n, sigma_other if s == OTHER else s) for (nf, r, c, n, s), _ in PINS]
    for (batch, want), octs in zip(PINS, plans(driver, batches)):
        for o, (rows, cols, var, *cap) in want.items():
            f = octs[o]
            assert (int(f["rows"]), int(f["cols"])) == (rows, cols), (batch, o)
            assert variant(f, tiles) == var, (batch, o, f)
            if cap:
                assert int(f["items"]) == int(f["cap"]) == cap[0], (batch, o, f)
        if batch[4] == OTHER:  # such a sigma0 reaches the dot2 strip kernels at octave 0: no tile widths, no difference-form taps
            assert all(f["ke"] not in tiles and f["hd"] == "0" for f in octs), batch


def test_diagnostics_switch_keeps_the_dot2_pass(driver):
    # VSLAM_HDIFF=0 (diagnostics build): the octaves of the difference form fall back to the dot2 choice of the same shape
    octs = plans(driver, [(256, 1080, 1920, 4, 1.6)], hdiff=0)[0]
    assert [variant(f, set()) for f in octs[2:]] == [("dot2", 16, 2, 1), ("dot2", 16, 1, 1)]


def test_tile_shape_choice(driver):
    # 1080p: octave 0 (2160 x 3840) takes the wide tile, octave 1 (1080 x 1920 = 7.5 tiles of 256) the tall one
    octs = plans(driver, [(1, 1080, 1920, 2, 1.6)])[0]
    assert [f["wide"] for f in octs] == ["1", "0"]


def test_gpu_case_table_selects_the_variants_it_names(driver):
    from tests.test_gpu_strip_variants import CASES

    tiles = tile_widths(driver)
    got = plans(driver, [(c.nf, c.rows, c.cols, c.n_octaves, c.sigma0) for c in CASES])
    seen = set()
    for c, octs in zip(CASES, got):
        assert sorted(c.variants) == list(range(c.n_octaves)) == list(range(len(octs))), c.id
        for o, f in enumerate(octs):
            assert variant(f, tiles) == c.variants[o], (c.id, o, f)
            seen.add(c.variants[o])
    assert {v[1:3] for v in seen if v[0] == "dot2"} == {(16, 4), (16, 2), (16, 1), (8, 4), (4, 4), (4, 1)}
    assert {v[-1] for v in seen if v[0] in ("dot2", "diff")} == {1, 2, 3, 6}
    assert {v[1] for v in seen if v[0] == "diff"} == set(range(1, 9))
    assert GENERIC in seen and TILE in seen
    # the pinned shapes are among the cases, each at a base sigma other than 1.6 where the pin says so, both of 1.2 and 2.0 in use
    shapes = {(c.nf, c.rows, c.cols): c for c in CASES}
    for (nf, r, cc, n, s), _ in PINS[1:]:
        c = shapes[(nf, r, cc)]
        assert (c.sigma0 != 1.6) == (s == OTHER) and c.n_octaves == (2 if s == OTHER else n), c.id
    assert {c.sigma0 for c in CASES} == {1.2, 1.6, 2.0}
