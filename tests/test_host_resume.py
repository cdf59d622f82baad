"""Host: the bookkeeping behind tests/test_gpu_resume.py, without a GPU.

An engine holds three derived copies of weights it does not own alone: params_bf16 and its transposes (of the student's arena) and
ema_bf16 (of the TEACHER's arena, read by the teacher forward of the student's engine).  Every model counts the edits made to its arena
from outside the native step (`_weights_version`, bumped by mark_weights_changed and everything that calls it); engine() compares the
student's count with the one its shadows were cast from and the teacher's count with the one the engine remembers, and calls
sync_shadows with bit 1, bit 2 or both.  A flag on the teacher module cannot do this: the teacher's own engine (a probe or an evaluate on
the teacher) clears it.  Here a stand-in engine records the sync_shadows calls; the casts themselves are tests/test_gpu_resume.py's.

The second half is the checkpoint file on the CPU: every arena and the step count come back bit for bit into objects that held other
values, with and without the `model_ema` flag.  The file takes 3 s."""
import copy
from types import SimpleNamespace

import pytest
import torch

from test_host_cpu import native, tiny_model  # noqa: F401  (the fixture builds the library)


class StandInEngine:
    """What VisionTransformerForCyclicalTraining.engine() reads of a NativeEngine, and a sync_shadows that records its argument."""

    def __init__(self, batch, teacher, adam_m, adam_v):
        self.batch, self.teacher, self.adam_m, self.adam_v = batch, teacher, adam_m, adam_v
        self.calls = []

    def sync_shadows(self, which=3):
        self.calls.append(which)


def other_state(model, shift):
    return {k: v + shift for k, v in model.state_dict().items() if v.dtype.is_floating_point}


def trainer(with_teacher=True):
    from uncertainty_vit_amd import utils
    model = tiny_model()
    ema = utils.ModelEmaV2(model, decay=0.5)
    m, v = torch.zeros_like(model._arena), torch.zeros_like(model._arena)
    model._engine = StandInEngine(3, ema.module if with_teacher else None, m, v)

    def engine():
        e = model.engine(3, teacher=ema.module, adam_m=m, adam_v=v) if with_teacher else model.engine(3)
        assert e is model._engine, "engine() replaced the engine"
        calls, e.calls = e.calls, []
        return calls

    engine()                                   # the stand-in starts without a record of what it was synced to
    assert engine() == []
    return model, ema, engine


def student_inplace(model, ema):
    with torch.no_grad():
        model._arena.mul_(1.01)
    model.mark_weights_changed()


EDITS = {
    "student_inplace": (student_inplace, 1),
    "student_load": (lambda model, ema: model.load_state_dict(other_state(model, 0.5), strict=False), 1),
    "student_flag": (lambda model, ema: setattr(model, "_shadows_stale", True), 1),                  # what older callers wrote
    "student_reinit": (lambda model, ema: model._init_weights(), 1),
    "student_apply": (lambda model, ema: model.float(), 1),                                          # _apply rebinds the arena
    "teacher_set": (lambda model, ema: ema.set(model), 2),
    "teacher_update": (lambda model, ema: ema.update(model), 2),
    "teacher_load": (lambda model, ema: ema.module.load_state_dict(other_state(model, 0.25), strict=False), 2),
    "teacher_mark": (lambda model, ema: ema.module.mark_weights_changed(), 2),
    "both": (lambda model, ema: (student_inplace(model, ema), ema.set(model)), 3),
}


@pytest.mark.parametrize("edit", list(EDITS))
def test_an_edit_leads_to_one_sync_with_its_bits(native, edit):  # noqa: F811
    """Each edit: exactly one sync_shadows call with the bits of what moved at the next engine() call, none at the one after; no edit, no
    call.  `_shadows_stale` keeps reading as the student's own state."""
    fn, bits = EDITS[edit]
    model, ema, engine = trainer()
    assert not model._shadows_stale
    fn(model, ema)
    assert model._shadows_stale == bool(bits & 1)
    assert engine() == [bits]
    assert not model._shadows_stale
    assert engine() == [] and engine() == []


@pytest.mark.parametrize("edit", ["teacher_set", "teacher_update", "teacher_load"])
def test_a_teacher_edit_survives_the_teachers_own_engine(native, edit):  # noqa: F811
    """The teacher module has an engine of its own (an eval forward on it) that syncs and clears the teacher's own state after the edit:
    the student's engine still has to refresh ema_bf16, once."""
    model, ema, engine = trainer()
    teacher = ema.module
    teacher._engine = StandInEngine(3, None, None, None)
    assert teacher.engine(3).calls == [3]
    EDITS[edit][0](model, ema)
    assert teacher._shadows_stale
    teacher._engine.calls = []
    assert teacher.engine(3).calls == [3] and not teacher._shadows_stale        # no teacher of its own: ema_bf16 is a cast of its own arena
    assert teacher.engine(3).calls == [3]
    assert engine() == [2]
    assert engine() == []
    teacher._shadows_stale = False                                               # the flag alone, cleared by hand: nothing to redo, nothing lost
    assert engine() == []


def test_a_model_without_a_teacher_syncs_both_copies(native):  # noqa: F811
    """Without a teacher the engine's ema_bf16 is a cast of the model's own arena (the eval forward's engine): an edit refreshes both."""
    model, _, engine = trainer(with_teacher=False)
    student_inplace(model, None)
    assert engine() == [3] and engine() == []


def test_a_copy_starts_unsynced_and_counts_on_its_own(native):  # noqa: F811
    model, ema, engine = trainer()
    twin = copy.deepcopy(model)
    assert twin._engine is None and twin._shadows_stale
    twin.mark_weights_changed()
    assert engine() == []                                                        # neither the student nor its teacher moved


def filled(seed, with_ema=True):
    from uncertainty_vit_amd import utils
    from uncertainty_vit_amd.optim_factory import ArenaAdamW
    g = torch.Generator().manual_seed(seed)
    m = tiny_model()
    ema = utils.ModelEmaV2(m, decay=0.5)
    opt = ArenaAdamW(m, lr=1e-3, weight_decay=0.05)
    opt._ensure_state()
    with torch.no_grad():
        for t in (m._arena, ema.module._arena, opt.exp_avg, opt.exp_avg_sq):
            t.copy_(torch.randn(t.shape, generator=g))
        opt.exp_avg_sq.abs_()
    return m, ema, opt


@pytest.mark.parametrize("teacher_flag", [True, False])
def test_checkpoint_restores_every_arena(native, tmp_path, teacher_flag):  # noqa: F811
    """save_model -> auto_load_model into objects that hold other values: student, both moments and the step count bit for bit; the teacher
    only with args.model_ema (utils.auto_load_model's docstring) -- without it the new teacher keeps what it held."""
    from uncertainty_vit_amd import utils
    m, ema, opt = filled(1)
    opt.step_count = 4
    args = SimpleNamespace(output_dir=str(tmp_path), auto_resume=True, resume="", start_epoch=0)
    utils.save_model(args, 6, m, m, opt, utils.NativeScalerWithGradNormCount(), model_ema=ema)
    m2, ema2, opt2 = filled(2)
    held = ema2.module._arena.clone()
    assert not torch.equal(m2._arena, m._arena) and not torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq) and opt2.step_count == 0
    if teacher_flag:
        args.model_ema = True
    versions = m2._weights_version, ema2.module._weights_version
    utils.auto_load_model(args, m2, m2, opt2, utils.NativeScalerWithGradNormCount(), model_ema=ema2)
    assert args.start_epoch == 7 and opt2.step_count == 4
    live = torch.zeros(m._arena.numel(), dtype=torch.bool)          # alignment pads belong to no state-dict entry: a file does not carry them
    for _, off, numel, _, _ in m._layout:
        live[off:off + numel] = True
    assert 0 < int((~live).sum()) < 64
    same = lambda a, b: torch.equal(a[live], b[live])  # noqa: E731
    assert same(m2._arena, m._arena) and same(opt2.exp_avg, opt.exp_avg) and same(opt2.exp_avg_sq, opt.exp_avg_sq)
    assert same(ema2.module._arena, ema.module._arena) if teacher_flag else torch.equal(ema2.module._arena, held)
    assert m2._weights_version > versions[0] and (ema2.module._weights_version > versions[1]) == teacher_flag
