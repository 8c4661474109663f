"""trainer.loss_slots: which slots of the loss vector (layout: include/discogan_hip.h, dg_loss_mix_fwd) carry gradient in a D-step /
G-step of each architecture.  The expected tuples are written out: they are the selection image_translation.py:374-382 makes."""
import pytest

from discogan_modernized_amd.trainer import DiscoGANTrainer, default_args, loss_slots


def _table(nfm):
    fmA, fmB = tuple(range(8, 8 + nfm)), tuple(range(8 + nfm, 8 + 2 * nfm))
    return {("discogan", True): (0, 7, (2, 3, 5, 6)),
            ("discogan", False): (0, 6, (0, 1, 4, 7) + fmA + fmB),
            ("recongan", True): (1, 7, (5, 6)),
            ("recongan", False): (1, 6, (0, 7) + fmB),
            ("gan", True): (2, 7, (5, 6)),
            ("gan", False): (2, 6, (7,) + fmB)}


@pytest.mark.parametrize("nfm", [1, 3])
@pytest.mark.parametrize("dstep", [True, False])
@pytest.mark.parametrize("arch", ["discogan", "recongan", "gan"])
def test_loss_slots_table(arch, dstep, nfm):
    assert loss_slots(arch, dstep, nfm) == _table(nfm)[(arch, dstep)]


def test_loss_slots_written_out():
    assert loss_slots("discogan", False, 3) == (0, 6, (0, 1, 4, 7, 8, 9, 10, 11, 12, 13))
    assert loss_slots("recongan", False, 3) == (1, 6, (0, 7, 11, 12, 13))
    assert loss_slots("gan", False, 1) == (2, 6, (7, 9))


@pytest.mark.parametrize("dstep", [True, False])
def test_unknown_model_arch_is_refused(dstep):
    with pytest.raises(ValueError, match="unknown model_arch cyclegan"):
        loss_slots("cyclegan", dstep, 3)


def test_trainer_refuses_an_unknown_model_arch_at_construction():
    # before anything is allocated on a device: this runs without one
    with pytest.raises(ValueError, match="unknown model_arch cyclegan"):
        DiscoGANTrainer(default_args(model_arch="cyclegan"), device="cuda", image_size=16, seed=1234)
