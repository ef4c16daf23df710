"""Which form of the relation head runs for a shape (spacap3d_amd/relation.py: tier): pure host logic over the library's
``*_supported`` predicates, so it needs the built library but no GPU."""
import pytest

# (H, K, D, C, NO, grad) -> form
PINS = [
    ((8, 256, 16, 128, 9, True), "fused"),          # the benchmark shape
    ((8, 8, 16, 128, 9, True), "fused"),
    ((8, 8, 16, 128, 9, False), "fused"),
    ((8, 255, 16, 128, 9, True), "wide"),           # K not a multiple of 8: the 128-wide head on the wide form
    ((8, 7, 16, 128, 9, True), "wide"),
    ((32, 512, 16, 512, 9, True), "wide"),          # the 512-wide / 32-head stress configuration
    ((4, 16, 32, 128, 9, True), "l1+tail"),
    ((4, 16, 32, 128, 9, False), "l1+tall"),        # the tail node exists for training only
    ((8, 16, 16, 128, 5, True), "l1+tall"),         # a last layer that is not 9 wide
    ((2, 16, 64, 128, 9, True), "feature+tail"),    # a head count without a first-layer kernel: feature + Linear
    ((2, 16, 64, 128, 9, False), "feature+tall"),
]


@pytest.mark.parametrize("shape,form", PINS)
def test_tier_names_the_form_that_runs(shape, form):
    from spacap3d_amd.relation import tier
    H, K, D, C, NO, grad = shape
    assert tier(H, K, D, C, NO, True, grad) == form
    assert tier(H, K, D, C, NO, False, grad) is None       # no form runs on the CPU


def test_moved_names_stay_importable_from_their_old_modules():
    from spacap3d_amd import attention, linear, relation
    for mod, names in ((attention, ("RelationFeature", "RelationLayer1", "relation_feature", "relation_layer1")),
                       (linear, ("RelationTail", "RelationHead", "RelationWide", "RelationU", "relation_tail", "relation_head_wide",
                                 "relation_head"))):
        for n in names:
            assert getattr(mod, n) is getattr(relation, n)
    with pytest.raises(AttributeError):
        linear.no_such_name
