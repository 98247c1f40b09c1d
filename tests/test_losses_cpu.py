"""CPU tests of the table of optional training losses (dtgan_amd.losses): what a captured step's key takes from the records,
and the refusals TrainOptions.parse runs over them."""
import pytest

import dtgan_amd  # noqa: F401
from dtgan_amd import losses, model as M
from model_cases import parse_train as _parse

# the options StepGraph._key named one by one before the records existed: every one must still be in the key
KEY_BEFORE = ["max_gnorm", "lambda_A", "lambda_B", "lambda_z_B", "lambda_sup_A", "lambda_sup_B", "stoch_enc", "z_gan", "beta1",
              "lambda_spec_A", "lambda_spec_B", "ema_decay", "lambda_marg_A", "lambda_marg_B", "lambda_ssim_A", "lambda_ssim_B",
              "lambda_crps_B", "crps_members", "crps_alpha", "lambda_fss_A", "lambda_fss_B", "fss_tau", "fss_loss_windows",
              "fss_loss_thr_A", "fss_loss_thr_B"]
OF_NO_FAMILY = ["max_gnorm", "lambda_A", "lambda_B", "lambda_z_B", "lambda_sup_A", "lambda_sup_B", "stoch_enc", "z_gan", "beta1",
                "ema_decay"]


class _Recorded(object):
    """options that note which of them are read"""

    def __init__(self, **kw):
        self.__dict__.update(kw, read=[])

    def __getattribute__(self, name):
        if not name.startswith("_") and name != "read":
            self.read.append(name)
        return object.__getattribute__(self, name)


def test_the_step_graph_key_holds_every_option_it_held_and_takes_the_families_from_their_records():
    import inspect
    import torch
    assert len(KEY_BEFORE) == len(set(KEY_BEFORE)) == 25

    class Net(object):
        training = True

    class Model(object):
        netG_A_B = Net()

        def _optimizers(self):
            return {}
    m = Model()
    m.opt = _Recorded(**dict((k, 0.0) for k in KEY_BEFORE))
    g = M.StepGraph(m)
    x = torch.zeros(2, 3, 4, 4)
    base = g._key(x, x, x)
    key = list(m.opt.read)                                        # the options the key reads, in its order
    assert sorted(key) == sorted(KEY_BEFORE)
    source = inspect.getsource(M.StepGraph._key)
    for name in KEY_BEFORE:                                       # the key spells the options of no family, and only those
        assert ('"%s"' % name in source) == (name in OF_NO_FAMILY), name
    from_records = losses.key_options()
    assert sorted(from_records) == sorted(set(KEY_BEFORE) - set(OF_NO_FAMILY))
    assert key == OF_NO_FAMILY + from_records                     # nothing of a family is spelled in the key itself
    for fam in losses.FAMILIES:
        assert set(fam.options()) | set(fam.reads) <= set(from_records), fam.stem
    assert losses.BY_STEM["crps"].options() == ["lambda_crps_B"]
    assert losses.BY_STEM["fss"].reads == ("fss_tau", "fss_loss_windows", "fss_loss_thr_A", "fss_loss_thr_B")
    # ... and the key itself: a changed weight, member count or threshold table is another key
    for name, value in (("lambda_fss_B", 0.5), ("crps_members", 2), ("fss_loss_thr_A", [[0.5, 1.0]]), ("fss_loss_windows", (3, 9)),
                        ("lambda_spec_A", 1.0), ("lambda_marg_B", 1.0), ("lambda_ssim_A", 1.0), ("ema_decay", 0.9)):
        setattr(m.opt, name, value)
        assert g._key(x, x, x) != base, name
        hash(g._key(x, x, x))
        setattr(m.opt, name, 0.0)
    assert g._key(x, x, x) == base


@pytest.mark.parametrize("fam", losses.FAMILIES, ids=lambda f: f.stem)
def test_the_parser_runs_the_common_refusals_from_the_record(tmp_path, capsys, fam):
    sup = ("--supervised",) if fam.paired_only else ()
    lo, hi, pow2, phrase = fam.grid
    for option in fam.options():
        flag = "--" + option

        def refused(*extra):
            with pytest.raises(SystemExit):
                _parse(tmp_path, *extra)
            err = capsys.readouterr().err
            assert flag in err, err
            return err
        assert getattr(_parse(tmp_path, *(sup + (flag, "0.25"))), option) == 0.25
        # a negative weight
        if fam.negative_ok:
            assert getattr(_parse(tmp_path, flag, "-0.25"), option) == -0.25       # spec: never refused, reads as off
        else:
            err = refused(flag, "-0.25")
            assert "negative" in err and "-0.25" in err
        # a term of the paired step alone: without --supervised, and in a model without a paired step
        if fam.paired_only:
            assert "--supervised" in refused(flag, "0.25")
            for model in ("cycle_gan", "stoch_cycle_gan"):
                err = refused("--supervised", flag, "0.25", "--model", model)
                assert "paired step" in err and model in err
        else:
            assert _parse(tmp_path, flag, "0.25", "--model", "stoch_cycle_gan").model == "stoch_cycle_gan"
        # the grid: both ends accepted, one past either end refused with the size and the record's phrase
        for size in (lo, hi):
            assert _parse(tmp_path, *(sup + (flag, "0.25", "--grid_size", str(size), "--batchSize", "1"))).grid_size == size
        for size in ([lo - 1] if lo > 1 else []) + [hi + 1, 2 * hi] + ([48] if pow2 else []):
            err = refused(*(sup + (flag, "0.25", "--grid_size", str(size))))
            assert phrase in err and "--grid_size %d" % size in err
        assert _parse(tmp_path, "--grid_size", str(2 * hi), flag, "0").grid_size == 2 * hi      # off: every size passes
