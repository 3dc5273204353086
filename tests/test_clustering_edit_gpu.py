"""Editing a held clustering on the GPU (DESIGN.md "Editing a held clustering"): a Clustering state on a real context next to the
same state driven by the stand-in engines of tests/fold_cases.py (the reference's loop and the fold in numpy).  After every step the
two hold the same members, ids and centroids, as bits."""
import numpy as np
import pytest

from tests import fold_cases as FC
from tests import ward_cases as WC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from imageclust_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


def stand_in(C, ss, mn, mx, kt, *extra):
    assert not extra
    return FC.seeded_engine(C, ss, mn, mx, kt)


def same(real, fake, step):
    a, b = FC.snapshot(real), FC.snapshot(fake)
    assert len(a[0]) == len(b[0]), (step, len(a[0]), len(b[0]))
    for q, (x, y) in enumerate(zip(a[0], b[0])):
        assert x == y, (step, q, x[0], y[0], x[2:], y[2:])
    assert a[1:] == b[1:], step


def test_every_edit_next_to_the_stand_ins(ctx):
    from imageclust_amd import clustering as CL

    E = WC.mog(300, 8, 31)
    ids = ["i%d" % i for i in range(300)]
    rng = np.random.default_rng(32)
    real = CL.Clustering.start(E, ids, 3, 6, ctx=ctx)
    fake = CL.Clustering.start(E, ids, 3, 6, engine=stand_in, fold_engine=FC.engine)
    same(real, fake, "start")
    gone = [ids[i] for i in rng.permutation(300)[:20]]
    for st in (real, fake):
        st.remove(gone)
    same(real, fake, "remove")
    assert ctx.last_fold_stats()["groups"] >= 1
    tgt = next(c for c in fake.clusters if len(c.Members) <= 3)
    pool = [k for c in fake.clusters if c is not tgt and len(c.Members) >= 4 for k in c.Members[1:3]]
    into, out = pool[:3], pool[3:5]
    for st in (real, fake):
        st.move(into, tgt.Members[0])
        st.move(out)
    same(real, fake, "move")
    for st in (real, fake):
        assert st.recluster()
    same(real, fake, "recluster")
    # a partition from elsewhere with a 14-member group, split by the state's own engine
    groups = [ids[10:24], ids[40:43], ids[50:56]]
    real = CL.Clustering.from_partition(E, ids, groups, 3, 6, ctx=ctx)
    fake = CL.Clustering.from_partition(E, ids, groups, 3, 6, engine=stand_in, fold_engine=FC.engine)
    same(real, fake, "from_partition")
    assert real.oversized() == [ids[10]]
    for st in (real, fake):
        st.split([ids[10]])
    same(real, fake, "split")
    for st in (real, fake):
        st.split([fake.clusters[0].Members[0], ids[50]], k_target=2)
        assert st.oversized() == [] and st.recluster()
    same(real, fake, "split with k_target, recluster")


def test_adopt_2300_groups_remove_and_resume_on_the_large_engine(ctx):
    """6 000 rows adopted as 2 300 groups: more seeds than icl_cluster_many_seeded holds, so recluster() is icl_cluster_seeded."""
    from imageclust_amd import clustering as CL

    E = WC.mog(6000, 8, 33)
    ids = ["i%d" % i for i in range(6000)]
    cut = np.concatenate([[0], np.cumsum([3] * 1400 + [2] * 900)])
    groups = [ids[a:b] for a, b in zip(cut[:-1], cut[1:])]
    assert len(groups) == 2300 > CL.MANY_SEEDED_MAX and cut[-1] == 6000
    real = CL.Clustering.from_partition(E, ids, groups, 3, 6, ctx=ctx)
    fake = CL.Clustering.from_partition(E, ids, groups, 3, 6, engine=stand_in, fold_engine=FC.engine)
    same(real, fake, "from_partition")
    assert ctx.last_fold_stats()["groups"] == 2300 and ctx.last_fold_stats()["rows"] == 6000
    gone = [ids[i] for i in np.random.default_rng(34).permutation(6000)[:50]]
    for st in (real, fake):
        st.remove(gone)
    same(real, fake, "remove")
    assert len(real.clusters) > CL.MANY_SEEDED_MAX
    for st in (real, fake):
        assert st.recluster()
    same(real, fake, "recluster")
    assert len(real.last_merges) > 0
