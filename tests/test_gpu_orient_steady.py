"""The batched filterKeypoints and SIFT kernels where a workgroup walks SEVERAL records, against the CPU oracle.

The other oracle tests of these stages run chunks of at most 44 frames on frames with a few hundred survivors per level:
the host sizes the grids from the chunk's frame count alone (8192 / nf workgroups per frame, eight times that for
k_orient_survivors_pk and k_sift_descriptors_batch), so every workgroup there sees one record and the loops' second
trip - the record prefetch two ahead, wave 1 staging the next patch while wave 0 reads the previous survivor's histogram,
stale patch registers between interior and border survivors, the descriptor kernel's missing end-of-record barrier, its
early return, its two filter forms sharing LDS - never runs.  Their coarse octaves carry no survivors at all.

Here every call has 256 frames, the benchmark's chunk: 256 workgroups per frame for the packed kernel and the descriptors, 32
for k_orient_survivors.  Nearly all frames are constant (empty lists: workgroups with nothing to do beside busy ones); the
few content frames (tests/orientcensus.py: uniform noise, and noise enlarged block-wise so that octaves 1-3 have keypoints)
are compared byte for byte with oracle.Pyramid: keypoint list, survivor count, oriented points, descriptors, defined flags.
tests/test_orient_census_cpu.py asserts, on the CPU, how many records and trips these frames put through each path; the
descriptor kernel's floors (trips, the kt form of octaves 2 and 3, ext <-> kt and undefined -> defined between consecutive
records of a workgroup) are met by the frames of the two tests below, whose descriptors are compared in full."""
import contextlib

import numpy as np
import pytest

import oracle
from tests import orientcensus as oc
from tests.test_gpu_batch import check_oriented_frame
from visualslam_amd import capi, synth

pytestmark = pytest.mark.gpu
NF = oc.STEADY_NF
DEV = "cuda:0"


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    capi.build()
    return torch


@contextlib.contextmanager
def variant(torch, fused):
    """A context of its own per arithmetic variant (tests/test_gpu_f32_variant.py), the oracle switched with it."""
    c = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    c.set_f32_fused(fused)
    try:
        with oracle.fma_variant(fused):
            yield c
    finally:
        c.close()


def run_steady(ctx, torch, shape, content, caps, sigma0):
    """One vslam_detect_batch_dev call of 256 frames, constant but for content = {position: image}; only the DoG list, the
    oriented list and the descriptors are asked for.  Returns (params, {output: {position: numpy slice}}, the counts of all frames)."""
    rows, cols = shape
    p = capi.default_params(rows, cols, n_octaves=4, sigma0=sigma0, localize=1, orient=1, **caps)
    L = capi.batch_layout(p)
    frames = torch.full((NF, rows, cols), int(synth.frame_np(1, 1, kind="constant")[0, 0]), dtype=torch.uint8, device=DEV)
    for f, img in content.items():
        frames[f] = torch.from_numpy(img).to(DEV)
    o = dict(pyramid=torch.empty((NF, L.pyramid_frame_bytes), dtype=torch.uint8, device=DEV),
             dog_points=torch.zeros((NF, p.dog_cap, 6), dtype=torch.int32, device=DEV), dog_counts=torch.full((NF,), -1, dtype=torch.int32, device=DEV),
             oriented_points=torch.zeros((NF, p.oriented_cap, 6), dtype=torch.int32, device=DEV),
             oriented_counts=torch.full((NF,), -1, dtype=torch.int32, device=DEV), oriented_survivors=torch.full((NF,), -1, dtype=torch.int32, device=DEV),
             descriptors=torch.full((NF, p.oriented_cap, 128), 7.0, dtype=torch.float32, device=DEV),
             descriptor_defined=torch.full((NF, p.oriented_cap), 9, dtype=torch.uint8, device=DEV))
    ctx.detect_batch(p, frames, **o)
    torch.cuda.synchronize()
    counts = {k: o[k].cpu().numpy() for k in ("dog_counts", "oriented_counts", "oriented_survivors")}
    out = {k: {f: v[f].cpu().numpy() for f in content} for k, v in o.items() if k != "pyramid"}
    return p, out, counts


def check_steady(p, out, counts, content):
    empty = np.array([f not in content for f in range(NF)])
    for k, v in counts.items():  # the constant frames: empty lists, whatever their neighbours hold
        assert not v[empty].any(), k
    for f, img in content.items():
        want = oracle.Pyramid(img, 4, p.sigma0)
        pts = [want.keypoints(o, p.extrema_window) for o in range(4)]
        allp = np.concatenate(pts)
        assert len(allp) <= p.dog_cap, "whole lists are compared: raise dog_cap"
        assert out["dog_counts"][f] == len(allp), (f, int(out["dog_counts"][f]), len(allp))
        assert out["dog_points"][f][: len(allp)].copy().view(capi.POINT_DTYPE).reshape(-1).tobytes() == allp.tobytes(), f
        check_oriented_frame(p, out, f, want, pts, 4)
        assert out["oriented_counts"][f] > 0
        want.close()


@pytest.mark.parametrize("sigma0,fused", [(1.6, False), (1.3, False), (1.6, True)])
def test_packed_kernel_in_steady_state(torch_mod, sigma0, fused):
    # k_orient_survivors_pk at 256 workgroups per frame and level: up to 4 (sigma0 = 1.6) / 6 (1.3) survivors per workgroup on
    # the noise frame, interior and border ones following each other at every patch alignment; the block-noise frame beside it
    # has one trip at level 1 and 4-5 at levels 2-3, and 8-14 trips of k_orient_survivors on octave 1.  sigma0 = 1.6: the
    # compiled-in tap counts 25 / 31 / 39; 1.3: the generic instantiation; fused: k_orient_survivors_pk<0, true>.
    content = {f: oc.steady_frame(name) for f, name in oc.PACKED_FRAMES.items()}
    with variant(torch_mod, fused) as ctx:
        p, out, counts = run_steady(ctx, torch_mod, oc.PACKED_SHAPE, content, oc.PACKED_CAPS, sigma0)
        check_steady(p, out, counts, content)


def test_coarse_octaves_through_k_orient_survivors(torch_mod):
    # production dispatch: octave 0 in the packed kernel, octaves 1-3 in k_orient_survivors at 32 workgroups per frame - patch
    # staged in LDS (octave 1, octave 2 levels 1-2), region without patch (octave 2 level 3), tap by tap (octave 3) - 2-3
    # survivors per workgroup; survivors on both sides of the flag word the two k_edge_flags launches share; descriptors of
    # octaves 2-3 in the kt form, next to ext-form ones in the same workgroup
    content = {f: oc.steady_frame(name) for f, name in oc.COARSE_FRAMES.items()}
    with variant(torch_mod, False) as ctx:
        p, out, counts = run_steady(ctx, torch_mod, oc.COARSE_SHAPE, content, oc.COARSE_CAPS, 1.6)
        check_steady(p, out, counts, content)


def test_octave_0_through_k_orient_survivors_at_sigma0_2(torch_mod):
    # sigma0 = 2.0: octave 0's widest span (64) is past the packed kernel's 60, so the noise frame's 703 survivors go through
    # k_orient_survivors: 22 per workgroup, interior (patch) and border ones in turn
    content = {128: oc.steady_frame("noise")}
    with variant(torch_mod, False) as ctx:
        p, out, counts = run_steady(ctx, torch_mod, oc.PACKED_SHAPE, content, oc.PACKED_CAPS, 2.0)
        check_steady(p, out, counts, content)
