"""recognize(), pixels in and an index out, against the oracle's fp64 pipeline.

The search tests assert exactness on the engine's own fp32 features.  This file asserts what a
caller sees: the row recognize() returns is the row of orc.project in fp64 followed by an fp64
ranking, for every probe whose fp64 top-2 margin exceeds a bound carried over from the
projection's tested error (parity_util, "Identity with the fp64 pipeline": the derivation), and
a row within that bound of the best for the others.  The engine projects the gallery and the
probes with its own kernel, in fp32 and in bf16.

tests/test_parity_generators_cpu.py checks on the reference alone that the probes' margins
straddle the bound: 100 noisy copies of gallery images far above it, and of 200 probes between
two gallery images at least 40 within 30 x the bound above it and at least 20 below it.  The
bf16 cosine bound exceeds every possible margin (see there), so that case asserts (b) alone.
"""
import numpy as np
import pytest

import parity_util as pu

pytestmark = pytest.mark.gpu


@pytest.fixture
def e(eng):
    """The session engine with the search options at their defaults before and after."""
    def reset():
        eng.set_option("search_split_bf16", 0)
        eng.set_option("search_prefix", 1)
        eng.set_option("search_prefix_split", 1)
    reset()
    yield eng
    reset()


@pytest.mark.parametrize("k,precision", pu.PIPELINE_CASES, ids=lambda v: str(v))
def test_recognize_is_the_fp64_pipeline_outside_the_projection_bound(e, k, precision):
    mean, w, gal, probes = pu.pipeline_case(k, precision)
    ref = pu.PipelineReference(mean, w, gal, probes, precision)
    e.set_model(mean, w, precision=precision)
    g = e.project(gal)
    # the premise, in the 2-norm: the projection is within its tested per-coordinate bounds
    assert (np.linalg.norm(g - ref.g, axis=1) <= ref.eps_g).all()
    e.set_gallery(g)
    for metric in ("l2", "cosine"):
        idx, _, feats = e.recognize(probes, metric, return_features=True)
        assert (np.linalg.norm(feats - ref.f, axis=1) <= ref.eps_p).all()
        vacuous = (precision, metric) == ("bf16", "cosine")
        sure = pu.assert_pipeline_identity(ref, metric, idx, min_guaranteed=0 if vacuous else
                                           pu.PIPELINE_NEAR + 40)
        assert vacuous or sure[:pu.PIPELINE_NEAR].all()
        # whatever the bound says (nothing, for bf16 cosine): a copy of a gallery image with noise
        # in -3..3 is recognised as that image, as test_recognize_bf16_agrees_with_fp32 expects
        np.testing.assert_array_equal(idx[:pu.PIPELINE_NEAR], np.arange(pu.PIPELINE_NEAR))
