"""GPU: kimimaro_amd.skeletonize_chunked on the two datasets of tests/chunked_ref.py -- equal, array for array, to the
composition it is defined as (per box the existing skeletonize, placement, simple_merge().consolidate(), host postprocess), to the
same composition made by the CPU oracle, and to itself whatever the lane count or the form of the dataset."""
import numpy as np
import pytest

import chunked_ref as R
import join_ref as J

pytestmark = pytest.mark.gpu

K = range(len(R.DATASETS))


@pytest.fixture(scope="module")
def eng():
    from kimimaro_amd.engine import Engine
    return Engine()


@pytest.fixture(scope="module")
def hip_run(eng):
    import kimimaro_amd
    return lambda labels, **kwargs: kimimaro_amd.skeletonize(labels, _engine=eng, progress=False, **kwargs)


def oracle_run(labels, **kwargs):
    from oracle import pipeline as P
    return P.skeletonize(labels, **kwargs)


def chunked(k, dataset=None, **kwargs):
    import kimimaro_amd
    kw = dict(teasar_params=R.TP, anisotropy=R.AN, dust_threshold=R.CHUNK_DUST, post_dust_threshold=R.POST_DUST, tick_threshold=R.TICK,
              width=2)
    kw.update(kwargs)
    return kimimaro_amd.skeletonize_chunked(R.dataset(k) if dataset is None else dataset, R.DATASETS[k][3], **kw)


@pytest.fixture(scope="module")
def hip_fragments(hip_run):
    return [R.fragments(R.dataset(k), R.DATASETS[k][3], hip_run) for k in K]


@pytest.fixture(scope="module")
def oracle_fragments():
    return [R.fragments(R.dataset(k), R.DATASETS[k][3], oracle_run) for k in K]


@pytest.fixture(scope="module")
def driver():
    return [chunked(k) for k in K]


@pytest.mark.parametrize("k", K)
def test_equals_its_own_composition(k, driver, hip_fragments):
    """(a) exact.  postprocess_many joins with kh_part_gaps, host postprocess with cKDTree: they agree wherever no join is decided
    by a tree_tie, which the statement of tests/join_ref.py shows first for EVERY label -- none is left out."""
    from kimimaro_amd import post
    for label, skel in R.fused(hip_fragments[k]).items():
        cleaned = post.remove_loops(post.remove_dust(skel.consolidate(remove_disconnected_vertices=True), R.POST_DUST))
        assert not J.join(cleaned, restrict_by_radius=True)[1], "label %d: a tree_tie decides a join" % label
    want = R.compose(hip_fragments[k], post.postprocess)
    several = [label for label, f in hip_fragments[k].items() if len(f) > 1]
    assert len(several) >= R.DATASETS[k][5]
    R.assert_same(driver[k], want)
    for label in several:
        assert len(driver[k][label].components()) == 1, label


@pytest.mark.parametrize("k", K)
def test_equals_the_oracle_made_composition(k, driver, oracle_fragments):
    """(b) vertices and edges exact, radii as tests/test_gpu_post.py compares the two"""
    from kimimaro_amd import post
    R.assert_same(driver[k], R.compose(oracle_fragments[k], post.postprocess), radii_rtol=1e-4)


def test_lane_count_does_not_matter(driver):
    """(c)"""
    timings = {}
    R.assert_same(chunked(0, width=1, timings=timings), driver[0])
    assert timings["chunks"] == R.DATASETS[0][4] and timings["fragments"] >= timings["chunks"] and timings["post_s"] > 0
    R.assert_same(chunked(0, width=3), driver[0])


def test_dataset_forms_give_equal_results(eng, driver):
    """(c) a tensor on the GPU, a C-ordered and a Fortran-ordered array"""
    lab = R.dataset(1)
    tensor = eng.torch.from_numpy(np.ascontiguousarray(lab).astype(np.int32)).to(eng.device)
    for form in (tensor, np.ascontiguousarray(lab), np.asfortranarray(lab)):
        R.assert_same(chunked(1, dataset=form), driver[1])


def test_dust_global(hip_run):
    """(d) the dataset-wide rule == the composition with object_ids and dust_threshold=0; 12 labels against 8 chunk by chunk"""
    from kimimaro_amd import post
    lab, chunk_shape = R.dataset(0), R.DATASETS[0][3]
    frags = R.fragments(lab, chunk_shape, hip_run, dust_threshold=R.GLOBAL_DUST, dust_global=True)
    assert len(frags) == 12
    R.assert_same(chunked(0, dust_threshold=R.GLOBAL_DUST, dust_global=True), R.compose(frags, post.postprocess))
    whole = chunked(0, dust_threshold=R.GLOBAL_DUST, dust_global=True, merge=False)
    per_chunk = chunked(0, dust_threshold=R.GLOBAL_DUST, merge=False)
    assert len(whole) == 12 and len(per_chunk) == 8 and set(per_chunk) < set(whole)
    assert 1003 not in whole and 1012 not in whole


def test_extra_target_in_the_second_chunk(driver):
    """(e) a voxel of the dataset inside the core of chunk 1 becomes a vertex of its label at f32(voxel) * anisotropy.  Ticks are
    not culled in this call: the branch to a chosen voxel is a tick like any other (on this dataset it is shorter than R.TICK)."""
    lab = R.dataset(0)
    point = (70, 20, 24)
    assert 48 <= point[0] < 96 and point[1] < 40
    label = int(lab[point])
    at = np.array(point, dtype=np.float32) * np.array(R.AN, dtype=np.float32)
    assert not (driver[0][label].vertices == at).all(axis=1).any()
    got = chunked(0, extra_targets_after=[point], tick_threshold=0)
    assert (got[label].vertices.view(np.uint32) == at.view(np.uint32)).all(axis=1).any()
    with pytest.raises(IndexError):
        chunked(0, extra_targets_after=[(96, 0, 0)])


def rows(vertices):
    return {tuple(r) for r in np.ascontiguousarray(vertices, dtype=np.float32).view(np.uint32).tolist()}


@pytest.mark.parametrize("k", K)
def test_fragments_meet_bit_for_bit_at_the_seams(k, hip_fragments, oracle_fragments):
    """(f) merge=False: the placed fragments, and the vertices that two fragments of a label share -- bit-equal float32 triples, the only
    ones consolidate() fuses -- are as many as the oracle's fragments share and lie on the planes two boxes have in common"""
    from kimimaro_amd.skeleton import Skeleton
    got = chunked(k, merge=False)
    assert list(got) == list(hip_fragments[k])
    an = np.array(R.AN, dtype=np.float32)
    planes = [{b[3][a] - 1 for b in R.boxes(R.DATASETS[k][0], R.DATASETS[k][3]) if b[3][a] < R.DATASETS[k][0][a]} for a in range(3)]
    assert planes[0] and planes[1]
    shared = 0
    for label, frags in got.items():
        assert len(frags) == len(hip_fragments[k][label])
        for a, b in zip(frags, hip_fragments[k][label]):
            assert a == b and a.id == label and a.space == "physical"
        for i in range(len(frags)):
            for j in range(i + 1, len(frags)):
                for bits in rows(frags[i].vertices) & rows(frags[j].vertices):
                    voxel = np.rint(np.array(bits, dtype=np.uint32).view(np.float32).astype(np.float64) / an).astype(int)
                    assert any(int(voxel[a]) in planes[a] for a in range(3)), (label, voxel)
        shared += sum(f.vertices.shape[0] for f in frags) - Skeleton.simple_merge(frags).consolidate().vertices.shape[0]
    seams = lambda fr: sum(sum(f.vertices.shape[0] for f in fs) - Skeleton.simple_merge(fs).consolidate().vertices.shape[0] for fs in fr.values())
    assert shared == seams(oracle_fragments[k]) and shared >= 20
