"""tests/component_scenes.py without a GPU: 64 scenes pinned by digest with their classes; the share of them the references
agree on (derivative_fuzz.qualify with the port oracle) and why the others are left out; what every class is for, read from
adjoint_reference.segment_lists alone (component_scenes.ray_statistics): no overlap beyond rounding where the parts lie
apart, touch or nest, a handful of rays deep in the overlap where they interpenetrate, the overlap of t x s on the rays of a
`window` scene, no exact tie of z_hi anywhere; the numpy restatements held to the 80-digit reference on a `deep` and an
`enclosed` scene (tests/test_derivative_references_cpu.py's machinery and bars) - their segment lists have not held
overlapping segments before; and the first seeds of the GPU sweeps (tests/test_gpu_component_fuzz.py), chosen here from the
draws alone.
"""
import numpy as np
import pytest

from course5_amd import meshgen as mg
from tests import component_scenes as cs
from tests import derivative_fuzz as df
from tests import test_derivative_references_cpu as refs

FIRST, N_SEEDS = 9000, 64

# seed: (class, sha256 of the scene)
PINNED = {
    9000: ("apart", "f321917f9e6861cf69534c2fc3d52ad6ab1635d6518833dbe827936c11b238bb"),
    9001: ("abutting", "082bc2ef41266ece09f955f3dff41379edf820ea8f05cb51085727b18472faa6"),
    9002: ("nested", "716029c73e31cd89a78901a5a3a82353e03a53ce80daae53c2002e741e76e279"),
    9003: ("deep", "0bd557edf6ed7fba5836f7a8cda1cda418203b310b7f8d6af7f80ddbe6597d33"),
    9004: ("enclosed", "b43e2e3ba862bb1a69d65094597bb271e603d3009b361f2c1ff6e45392d228a7"),
    9005: ("flush", "49357e502855a607d7d3e1aff4a9b3335d3218761d8bfaf9c5fe14b274179590"),
    9006: ("window", "1af7462c66cf779a239f07d26d0dd9cc7c26e2a19b68f79313ebf38012364937"),
    9007: ("three", "fa5a03a983595518a8989bede14ab20d3808befa6c6605f2981a5c940c0ff5bc"),
    9008: ("apart", "227e9e9182b9c7fb234a3dbd2a583f11841b3f5cf13688b7fb6926d67501a0f3"),
    9009: ("abutting", "c4600acbe6e25f934d908ea29db1238401cb661cd02b7ed420d459e3c1891c56"),
    9010: ("nested", "6af8e2cd11ae378df2af45483777919c4cfc80f6ac9ef2b83bb64e8067e6775e"),
    9011: ("deep", "7309603d06171cd0cc4f3e3da2ca8ea71e30780c95f87065ace5e2a5cbbd4fad"),
    9012: ("enclosed", "290955524d1a0d452ee38acd4ecbf52ff9762a5e3ba24b94db65f3cc6d0f80c1"),
    9013: ("flush", "908092a226d00fee3b38c70ee445532fe4f968f243fa0516feb56e40f845bb9a"),
    9014: ("window", "20f6ec8f0280f5acb3c6f3a1186b14e4ceb963eb12c8aecc3880fc3681e38775"),
    9015: ("three", "7a1903e85cf2e209a9a8a840b5d4adada5755b86c91df4c960f6577e34267c2d"),
    9016: ("apart", "eab533226c6d81759c784a8920f9d64ceb990ffe5278af47f30803ca1adac2c9"),
    9017: ("abutting", "6cac490b99a6ff34d096fac3158104b6a7a1d33972e78f02659c8f1e416a9dc5"),
    9018: ("nested", "4b54de1dcbb5cbd14d71b98b41ba36cd1b4e7b7dfc5715222136a4ca0735009b"),
    9019: ("deep", "222da364352728d77624fd9f230651adbc03070726aa0c1ad5881f5d79fa5e58"),
    9020: ("enclosed", "0ce49f3e342e86b9fd208989c4e7638224f09750b773e8191a7062e864316ee4"),
    9021: ("flush", "9da461e99860d9099b603a86524ae34719ed7ae4fde54f656b105c60f60addfa"),
    9022: ("window", "b4b2ac8763a4a04e3a06eda9a11c51ae1bc4f24a4fc160752bdbc5ebdece20d0"),
    9023: ("three", "018e2afa793fb2190754e9ad1f0777f177ce1090618e4d2575f4eda5b8e55806"),
    9024: ("apart", "ea1ef4ace3c4082714cebba563b1ba97958e7805d04ed73f4cc5f8c1d2b600eb"),
    9025: ("abutting", "417e974eb2445b647950a6c9fdaa2b0afdbdad4e9306a7d53c756029bad84c54"),
    9026: ("nested", "62727b06b4753c172cb0966b4bf219e54d436c3e2b755884d6123d8189f2631a"),
    9027: ("deep", "cf0fd065910784c9f01351083294418ea0624a29342c04e9d67f69df6b80dcb7"),
    9028: ("enclosed", "f7a09371d2d68cce413ba6cfbcc09362dceb304339bb06c41af7b49fb615df7b"),
    9029: ("flush", "67f70d32625ca9c656d015bc9207ab80742da09bdd77a09a5759a5234605ea47"),
    9030: ("window", "8a4f46c322a7a53e7fc070b415405ba8b51b63de77136d83aa34a382fc3fa96a"),
    9031: ("three", "d2924e643d9970d6a2bc2b503fbf2ca0e506b53eb10f96db46e619ecdc6dd73a"),
    9032: ("apart", "727667c5122a363ad65d33dcb4862c92daf2f4f0fd81fb727774a860ba777d8b"),
    9033: ("abutting", "52afc7c6e3267f91e11d141c91f7b498626dc400b381941eab0cf5ba76ffacc9"),
    9034: ("nested", "f34daea4b9516a668888d575248ffde837ab64dd18c717de722b452cdb85246b"),
    9035: ("deep", "086f5c82bc724fccbd1041f38a6d24ecd5e7845f2496c0828daf3800644a8e98"),
    9036: ("enclosed", "8638d0933179f2bfab6b3f3003a34264216edcba8acd5afbe8d62d2c62127015"),
    9037: ("flush", "b11e2cacb60e7c65b0dd07533fccfd97586639f09f7fc05fd134335d474660d8"),
    9038: ("window", "97487b04ed088394050cd13e226f8a2b87dee7c80c4daf5070f8e8a402b94ce3"),
    9039: ("three", "ef695aa00a0eb318ef33ba90fac15c9b76f47c9829fe1495af3eb7625c56799f"),
    9040: ("apart", "98251eaaefd33d0d284437a3d6e62fb3a2556a7890a15908254b5c0582f663b6"),
    9041: ("abutting", "01519011e4f52d58e1ab9d0a80975b93f0fb7d1757add863b033b3234f60efb2"),
    9042: ("nested", "f29ee82c213bd4ad8ae7a781f8fe73c16dcbd82e3678febf7138ea38221cf91d"),
    9043: ("deep", "51425e00eddf6ef2a14b80521f4df2cfd9019544865f60db9adea3082ddac498"),
    9044: ("enclosed", "40c096860eae5b49d798bcc82543c22b572470f381dfdc71f9c4cbf7975f32f9"),
    9045: ("flush", "10f2c5a13f0fdf403d545bd440a8f2d01e912b9ea806241a2d96c7150f49e468"),
    9046: ("window", "c72cdb1a1c9d2ca9ed404fbfd8772a6e7134061b0e0b6394e7531d2b55df4301"),
    9047: ("three", "ce65250ef606e68b0e0ba7cf746647eaabd9f92609a3579ecdd29442612c260f"),
    9048: ("apart", "c8cdbfb28bc3c61930cace34961d48b84f43d394b45fea071d1443a52163d33d"),
    9049: ("abutting", "c84a5631b124acdc934ed3ab5fc63be7cc69f9b7c6162093be04a6d2223a8bcc"),
    9050: ("nested", "6b4d362e0168c0d230f325fb50c86b123d8bc1a09ee3a0e435d6a73c1384894c"),
    9051: ("deep", "5ae67baa3ab6b86b43e448266490deeda4bd505fec14ab85192afeb27be3a3e6"),
    9052: ("enclosed", "b168548642d3a011fdfee386b7229a06bc4bc581c03eeb10e51cf432b3dc3d5b"),
    9053: ("flush", "eeee59111c13f78c33b73e54575079d3d06e3852725573c3222375503223a081"),
    9054: ("window", "335fa028f4693f6f60417245df556825f14f933cfc4f9ca690929fb168723d21"),
    9055: ("three", "bdb68b70a40aaebe2bc733eccf5c694297b352f7bce75ebf5492af9d46c8faf0"),
    9056: ("apart", "e4770df4ef16056ad42227b376963102074abdb15da45d4b461fcebcf10d59fd"),
    9057: ("abutting", "469ec073402a9bae9ac015e7185de40b3d370b437ed2e9df6c5954a8c1c79119"),
    9058: ("nested", "90a86e7cf398e8f00a2a55768453719929a25d9200ec7ec11c09e52bd9b2e6f4"),
    9059: ("deep", "4e32c3810bb74e3fe9aa4e14579a0b9ac80c0b43d6a0534e86c12dd2df58a745"),
    9060: ("enclosed", "39e3a483fe0562f063a55fc724155969e44c580cd95134e02cad2998eac1d6d8"),
    9061: ("flush", "b0eaf577974bf8a80524d306a04e0f7cf40f04dfe0cb1bb6baa59da1c772cda6"),
    9062: ("window", "32379e0f59f392c8c5eae50b57db1e563a4af3c751777c26738e4ed43e5f94fd"),
    9063: ("three", "d53ca62c1696f1e98ccd2e396d2bf47a0f936091fdd6f7d2a2e97aa5cee56c9d"),
}


@pytest.mark.parametrize("seed", sorted(PINNED))
def test_the_component_scenes_have_not_changed(seed):
    assert (cs.describe(seed)["class"], cs.digest(seed)) == PINNED[seed]


def test_the_classes_go_by_the_seed_and_the_scenes_are_what_they_say():
    assert sorted(PINNED) == list(range(FIRST, FIRST + N_SEEDS))
    for seed in range(FIRST, FIRST + N_SEEDS):
        d = cs.describe(seed)
        xyz, cells, alpha, q, _rots, (rx, ry), limit = cs.scene(seed)
        part = cs.part_of_cell(seed)
        assert d["class"] == cs.CLASSES[seed % 8]
        assert 30 <= rx <= 100 and 24 <= ry <= 80 and 0.5 <= limit < 6
        assert cs.MIN_CELLS <= len(cells) <= cs.MAX_CELLS and len(alpha) == len(q) == len(cells) == len(part)
        assert len(d["parts"]) == (3 if d["class"] == "three" else 2) and all(2 <= p["n"] <= 4 for p in d["parts"])
        assert (mg.signed_volumes(xyz, cells) > 0).all()
        assert np.array_equal(np.unique(cells), np.arange(len(xyz))), (seed, "unused points")
        # the parts share no point id
        owner = np.full(len(xyz), -1)
        for p in range(len(d["parts"])):
            ids = np.unique(cells[part == p])
            assert (owner[ids] == -1).all(), (seed, "two parts share a point id")
            owner[ids] = p
        # a pixel inside the border under ANY view: inside the ball about the point every view turns the grid about
        assert np.sqrt(((xyz - np.array([1.0, 0.0, 0.0])) ** 2).sum(1)).max() <= cs.RADIUS * (1 + 1e-9)
        assert d["slack"] == cs.slack(xyz)
        if d["class"] == "window":
            assert d["t"] == cs.WINDOW_T[(seed // 8) % 6]
        if d["class"] == "three":
            assert all(c in cs.THREE_CLASSES for c in d["pairs"])
    assert {cs.describe(seed)["t"] for seed in range(FIRST, FIRST + 48) if seed % 8 == 6} == set(cs.WINDOW_T)


def test_abutting_sides_are_coplanar_to_the_bit_before_the_view():
    for seed in range(FIRST, FIRST + N_SEEDS):
        if cs.CLASSES[seed % 8] != "abutting":
            continue
        xyz, cells = cs.scene(seed)[:2]
        part = cs.part_of_cell(seed)
        a, b = xyz[np.unique(cells[part == 0])], xyz[np.unique(cells[part == 1])]
        # along one axis of object space the two boxes meet at ONE double: A ends where B begins
        meet = [k for k in range(3) if a[:, k].max() == b[:, k].min() or b[:, k].max() == a[:, k].min()]
        assert len(meet) == 1, (seed, meet)
        k = meet[0]
        wall = a[:, k].max() if a[:, k].max() == b[:, k].min() else a[:, k].min()
        # ... and the lattices do not match: the points of the two facing sides differ
        fa, fb = a[a[:, k] == wall], b[b[:, k] == wall]
        assert len(fa) >= 9 and len(fb) >= 9
        assert {tuple(p) for p in fa} != {tuple(p) for p in fb}


class _Family:
    """The 64 scenes, each drawn and qualified once."""

    def __init__(self, oracle):
        self.oracle, self.rows = oracle, None

    def all(self):
        if self.rows is None:
            self.rows = []
            for seed in range(FIRST, FIRST + N_SEEDS):
                s = df.derivative_scene(seed, cs.scene)
                d = cs.describe(seed)
                d.update(seed=seed, why=df.qualify(s, self.oracle), soup=s.soup)
                self.rows.append(d)
                print(f"seed {seed}: {cs.describe_line(seed)}; {s.res[0]}x{s.res[1]}" + (f" - not used: {d['why']}" if d["why"] else ""))
        return self.rows


@pytest.fixture(scope="module")
def family(oracle_port):
    return _Family(oracle_port)


def test_the_references_agree_on_nine_scenes_in_ten(family):
    left_out = [d for d in family.all() if d["why"]]
    print(f"{N_SEEDS - len(left_out)} of {N_SEEDS} seeds used; not used: " + "; ".join(f"{d['seed']} ({d['why']})" for d in left_out))
    assert N_SEEDS - len(left_out) >= 0.9 * N_SEEDS
    assert not [d["seed"] for d in left_out if "segment_lists gives" in d["why"]]  # (none for a disagreement of the references)


def test_every_class_shows_what_it_is_for():
    for seed in range(FIRST, FIRST + N_SEEDS):
        d = cs.describe(seed)
        over = d["overlaps_in_s"]
        assert d["ties"] == 0, (seed, "an exact tie of z_hi within a pixel")
        assert d["overlapping"] == bool((over > 2.0).any())
        if d["class"] in ("apart", "abutting", "nested"):
            assert d["overlap_rays"] == 0, (seed, d["class"], d["overlap_rays"], d["max_overlap_in_s"])
        if d["class"] in ("deep", "enclosed", "flush"):
            assert int((over > 4.0).sum()) >= 8, (seed, d["class"], int((over > 4.0).sum()))
        if d["class"] == "window":
            t = d["t"]
            assert int((np.abs(over - t) <= 0.1 * t).sum()) >= 8 and not (over > 2.0 * t).any(), (seed, t, over)
            assert d["overlapping"] == (t > 2.0)
    # (a gap shows only on rays that cross both parts, and not below rounding: in most of the scenes, not in every one)
    gaps = [cs.describe(seed)["gap_rays"] > 0 for seed in range(FIRST, FIRST + N_SEEDS) if cs.CLASSES[seed % 8] in ("apart", "nested")]
    assert sum(gaps) >= 0.5 * len(gaps)


def test_gaps_below_the_slack_are_drawn():
    gaps = [(cs.describe(seed)["placement"][0]["gap"], cs.describe(seed)) for seed in range(FIRST, FIRST + 256, 8)]
    print(sorted(g / 3.0 for g, _d in gaps))
    assert sum(g / 3.0 < 2.0 ** -24 for g, _d in gaps) >= 3 and sum(g / 3.0 > 2.0 ** -10 for g, _d in gaps) >= 3


# ---- the restatements against 80 digits, on lists with overlapping segments ------------------------------------------------

SEEDS = {"deep": 9003, "enclosed": 9004}


@pytest.mark.parametrize("kind", sorted(SEEDS))
def test_restatements_against_80_digits(kind, oracle_port):
    seed = SEEDS[kind]
    d = cs.describe(seed)
    assert d["class"] == kind and d["overlapping"]
    seen = refs._against_80_digits(seed, oracle_port, cs.scene)
    print(cs.describe_line(seed))
    for r, what, _ in seen["worst"]:
        assert r <= 64, (what, r)


@pytest.mark.parametrize("kind", sorted(SEEDS))
def test_geometry_restatements_against_80_digits(kind, oracle_port):
    assert refs.N_PIXELS == 90
    refs._geometry_against_80_digits(SEEDS[kind], oracle_port, cs.scene, False)
    print(cs.describe_line(SEEDS[kind]))


# ---- the GPU sweeps' seeds (tests/test_gpu_component_fuzz.py) ----------------------------------------------------------

def _first_seeds(n_sweeps, per_sweep):
    """From the draws alone: the first runs of per_sweep seeds beyond the pinned ones, beginning at a multiple of 8, in which
    every class occurs at least once on a scene that is no soup (derivative_scene turns one scene in five into a soup on
    "algorithm" 1, which bypasses the detection of overlapping parts)."""
    soup = {}
    found, at = [], FIRST + N_SEEDS
    while len(found) < n_sweeps:
        for seed in range(at, at + per_sweep):
            if seed not in soup:
                soup[seed] = df.derivative_scene(seed, cs.scene).soup
        if all(any(not soup[seed] for seed in range(at, at + per_sweep) if seed % 8 == k) for k in range(8)):
            found.append(at)
            at += per_sweep
        else:
            at += 8
    return found


def test_the_sweeps_begin_where_every_class_has_a_scene_that_is_no_soup(oracle_port):
    from tests import test_gpu_component_fuzz as gpu
    per_sweep = gpu.BLOCKS * gpu.PER_BLOCK
    assert per_sweep == 16
    firsts = [gpu.SWEEPS[name][0] for name in ("forward", "scalar", "geometry", "second_order", "vertex_exact")]
    assert firsts == _first_seeds(5, per_sweep) == [9064, 9080, 9104, 9120, 9136]
    for name, first in zip(sorted(gpu.SWEEPS), sorted(firsts)):
        used = set()
        left_out = 0
        for seed in range(first, first + per_sweep):
            s = df.derivative_scene(seed, cs.scene)
            why = df.qualify(s, oracle_port)
            left_out += why is not None
            assert why is None or "segment_lists gives" not in why, (seed, why)
            if why is None and not s.soup:
                used.add(cs.describe(seed)["class"])
        assert left_out <= 0.1 * per_sweep and used == set(cs.CLASSES), (first, left_out, used)
