"""GPU: the classifier input of InceptionV3Features and the label / logit plumbing of StoryRunner (rcdms_amd.scores).

  preprocess="pillow"   preprocessed_rows equals Pillow's resize((299, 299), BILINEAR) -> (u8 / 255 - mean) / std in float32 -> f16
                        bit for bit, pad channels +0, on 48 x 64 and 17 x 301 frames, on frames 1 and 3 of a strip read by pitch
                        and stride, with the ImageNet constants and with the transform_input-folded ones (that the kernel's
                        products and torchvision's divisions round alike for every byte is tests/test_scores_host.py's); the logits of the
                        whole network move with the input.  preprocess="fid" keeps the bits of the written-out FID resize of
                        tests/inception_oracle.py, to which the parent's kernel is held.  Two frame sizes share one plan.
  StoryRunner           label_counts after one call equals LabelCounts.update on classifier(res.videos, return_logits=True) by
                        hand; label_frames=(1, 2, 3, 4) drops frame 0; logit_bank rows equal
                        inception(videos, return_logits=True)[1] bit for bit, from the one forward; without the new keywords
                        the library calls and the plan counters are those of the same call on a runner without a classifier;
                        the refusals come before anything is launched."""
import numpy as np
import pytest
import torch

from tests import inception_oracle as IO
from tests import scores_oracle as O
from tests.test_hip_inception import counted, minus
from tests.test_story_gpu import DEV, S, chain  # noqa: F401  (chain: the module-scoped fixture)
from tests.test_story_metrics_gpu import call

pytestmark = pytest.mark.gpu
CLASSES = 9


@pytest.fixture(scope="module")
def nets(hiplib):
    """The FID network and a character classifier: different weights, both with a 9-row fc."""
    from rcdms_amd.inception import InceptionV3Features
    fid = InceptionV3Features(IO.synthetic_state_dict(0, num_classes=CLASSES), device=DEV)
    clf = InceptionV3Features(IO.synthetic_state_dict(1, num_classes=CLASSES), variant="torchvision", device=DEV, preprocess="pillow")
    return fid, clf


def pillow_rows(frames, mean, std):
    """frames: numpy uint8 (n, H, W, 3) -> float16 (n, 299, 299, 3) as torchvision's Resize -> ToTensor -> Normalize make them."""
    from PIL import Image
    m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    out = []
    for f in frames:
        r = np.asarray(Image.fromarray(f).resize((299, 299), Image.BILINEAR)).astype(np.float32)
        out.append(((r / np.float32(255.0) - m) / s).astype(np.float16))
    return np.stack(out)


def test_pillow_preprocess_bit_for_bit(nets):
    from rcdms_amd import inception as I
    fid, clf = nets
    g = torch.Generator().manual_seed(1)
    small = torch.randint(0, 256, (2, 48, 64, 3), generator=g, dtype=torch.uint8)
    thin = torch.randint(0, 256, (1, 17, 301, 3), generator=g, dtype=torch.uint8)
    strip = torch.randint(0, 256, (48, 5 * 64, 3), generator=g, dtype=torch.uint8)
    cells = strip.view(48, 5, 64, 3).permute(1, 0, 2, 3)                      # the five frames of the strip, by pitch
    folded = I.InceptionV3Features.__new__(I.InceptionV3Features)             # the same extractor under the folded constants
    folded.__dict__.update(clf.__dict__)
    folded.mean, folded.std = I.TRANSFORM_INPUT_MEAN, I.TRANSFORM_INPUT_STD
    for net in (clf, folded):
        for host, dev in ((small, small.to(DEV)), (thin, thin.to(DEV)), (cells[1:4:2].contiguous(), cells.to(DEV)[1:4:2])):
            got = net.preprocessed_rows(dev)
            assert tuple(got.shape) == (host.shape[0], 299, 299, 8) and got.dtype == torch.float16
            want = torch.from_numpy(pillow_rows(host.numpy(), net.mean, net.std))
            assert torch.equal(got[..., :3].cpu().view(torch.int16), want.view(torch.int16))
            assert not bool((got[..., 3:].view(torch.int16) != 0).any()), "pad channels are not +0"
    assert not cells.to(DEV)[1:4:2].is_contiguous()
    # "fid" keeps the written-out FID resize, bit for bit
    rows = fid.preprocessed_rows(small.to(DEV))
    assert torch.equal(rows[..., :3].cpu().view(torch.int16), IO.resize(small).permute(0, 2, 3, 1).half().view(torch.int16))
    assert not bool((rows[..., 3:].view(torch.int16) != 0).any())
    # the network sees the other input; two frame sizes share one plan
    built = clf.plans_built
    feats, logits = clf(small.to(DEV), return_logits=True)
    assert tuple(logits.shape) == (2, CLASSES) and bool(torch.isfinite(logits).all())
    built = clf.plans_built
    other = clf(torch.randint(0, 256, (2, 17, 301, 3), generator=g, dtype=torch.uint8).to(DEV))
    assert clf.plans_built == built and tuple(other.shape) == (2, 2048)
    as_fid = I.InceptionV3Features.__new__(I.InceptionV3Features)
    as_fid.__dict__.update(clf.__dict__)
    as_fid.preprocess = "fid"
    assert not torch.equal(as_fid(small.to(DEV)), feats)
    for kw in ({"preprocess": "pil"}, {"mean": (0.5, 0.5, 0.5)}, {"preprocess": "pillow", "std": (0.5, 0.0, 0.5)},
               {"preprocess": "pillow", "mean": (0.5, 0.5)}):
        with pytest.raises(ValueError, match="preprocess|mean and std"):           # before the state dict is looked at
            I.InceptionV3Features({}, device=DEV, **kw)


def test_story_runner_labels_and_logits(chain, nets):
    from rcdms_amd.kid import FeatureBank
    from rcdms_amd.scores import LabelCounts
    from rcdms_amd.story import StoryRunner
    b, (fid, clf) = chain, nets
    old = b.runner
    args = (old.prior_pipe, old.stage2_pipe, old.image_encoder)
    kw = dict(clip_processor=old.clip_processor, frame_transform=old.frame_transform)
    labels = torch.from_numpy(O.label_inputs(CLASSES, 5 * S, 11)[1]).view(S, 5, CLASSES)
    try:
        b.runner = StoryRunner(*args, inception=fid, classifier=clf, **kw)
        assert b.runner.classifier is clf and old.classifier is None
        call(b, (), labels=labels, label_counts=LabelCounts(CLASSES, DEV), logit_bank=FeatureBank(CLASSES, DEV), feature_source="inception",
             feature_banks=(FeatureBank(2048, DEV), FeatureBank(2048, DEV)))         # steady state: plans, tables, the black / white embeddings
        counts, some, bank = LabelCounts(CLASSES, DEV), LabelCounts(CLASSES, DEV), FeatureBank(CLASSES, DEV)
        gen, ref = FeatureBank(2048, DEV), FeatureBank(2048, DEV)
        res, c_all = counted(lambda: call(b, (), labels=labels, label_counts=counts, logit_bank=bank, feature_source="inception",
                                          feature_banks=(gen, ref)))
        videos = res.videos.reshape(5 * S, *res.videos.shape[2:])
        # the counts: what LabelCounts.update makes of the classifier's logits by hand
        logits = clf(videos, return_logits=True)[1]
        want = LabelCounts(CLASSES, DEV).update(logits.view(S, 5, CLASSES), labels.to(DEV))
        assert int(counts.state()[0]) == 5 * S and torch.equal(counts.state(), want.state())
        assert np.array_equal(counts.state().cpu().numpy(), O.label_state(logits.cpu().numpy(), labels.view(-1, CLASSES).numpy()))
        # the logits of the FID network, from the forward that made the features
        feats, fid_logits = fid(videos, return_logits=True)
        assert len(bank) == 5 * S and torch.equal(bank.rows(), fid_logits) and torch.equal(gen.rows(), feats)
        _, c_feats = counted(lambda: call(b, (), feature_source="inception", feature_banks=(FeatureBank(2048, DEV), FeatureBank(2048, DEV))))
        _, c_clf = counted(lambda: (clf(videos, return_logits=True), LabelCounts(CLASSES, DEV).update(logits, labels.view(-1, CLASSES).to(DEV))))
        _, c_fc = counted(lambda: fid(videos, return_logits=True))
        _, c_nofc = counted(lambda: fid(videos))
        extra = minus(c_all, c_feats)
        print(f"labels + logits on top of the Inception features: {extra}")
        assert extra == {k: c_clf.get(k, 0) + c_fc.get(k, 0) - c_nofc.get(k, 0) for k in extra}        # one classifier forward, one fc: no second FID forward
        assert extra.get("rcdm_label_counts") == 1 and extra.get("rcdm_conv2d") == c_clf["rcdm_conv2d"]
        # frames 1 .. 4 only
        res2 = call(b, (), labels=labels, label_counts=some, label_frames=(1, 2, 3, 4))
        assert torch.equal(res2.videos, res.videos)
        keep = LabelCounts(CLASSES, DEV).update(logits.view(S, 5, CLASSES)[:, 1:], labels.to(DEV)[:, 1:])
        assert int(some.state()[0]) == 4 * S and torch.equal(some.state(), keep.state()) and not torch.equal(some.state(), counts.state())
        # a second call adds
        call(b, (), labels=labels, label_counts=some, label_frames=(0,))
        assert torch.equal(some.state(), counts.state())
        # defaults: the calls and the plan counters of a runner that has no classifier
        plans = (fid.plans_built, clf.plans_built)
        _, c_with = counted(lambda: call(b, ()))
        assert (fid.plans_built, clf.plans_built) == plans
        b.runner = old
        call(b, ())                                                                # its own black / white embeddings, once
        _, c_without = counted(lambda: call(b, ()))
        b.runner = StoryRunner(*args, inception=fid, classifier=clf, **kw)
        assert not minus(c_with, c_without), minus(c_with, c_without)
        assert "rcdm_label_counts" not in c_with and "rcdm_conv2d" not in c_with
        # refusals, all before a launch
        bad = [
            dict(label_counts=counts),                                                        # no labels
            dict(labels=labels),                                                              # no counts
            dict(labels=labels[:, :, :8], label_counts=counts),                               # width
            dict(labels=labels, label_counts=LabelCounts(7, DEV)),
            dict(labels=labels[:1], label_counts=counts),
            dict(labels=labels.float(), label_counts=counts),
            dict(labels=labels, label_counts=counts, output_type="tensor"),
            dict(labels=labels, label_counts=counts, stage2=False),
            dict(labels=labels, label_counts=counts, label_frames=(1, 1)),
            dict(labels=labels, label_counts=counts, label_frames=(5,)),
            dict(labels=labels, label_counts=counts, label_frames=()),
            dict(logit_bank=bank),                                                            # feature_source is "clip"
            dict(logit_bank=FeatureBank(7, DEV), feature_source="inception"),
            dict(logit_bank=bank, feature_source="inception", output_type="tensor"),
        ]
        before = (counts.state().clone(), len(bank))
        for kwargs in bad:
            _, c = counted(lambda: pytest.raises(ValueError, call, b, (), **kwargs))
            assert not c, (kwargs, c)
        b.runner = StoryRunner(*args, inception=fid, **kw)
        _, c = counted(lambda: pytest.raises(ValueError, call, b, (), labels=labels, label_counts=counts))       # no classifier
        assert not c
        b.runner = StoryRunner(*args, classifier=clf, **kw)
        _, c = counted(lambda: pytest.raises(ValueError, call, b, (), logit_bank=bank, feature_source="inception"))   # no extractor
        assert not c
        assert torch.equal(counts.state(), before[0]) and len(bank) == before[1]
    finally:
        b.runner = old
