"""The model <-> engine binding protocol, once: EngineBound is the base of every torch module that an engine handle executes
(Siren, FourierNet, WaveletSiren, FeatherNet).

A bound module only OWNS NAMES AND SHAPES: every Parameter of `_param_list()` (and its .grad) is a zero-copy view of the
handle's flat fp32 state, so optimiser / masking / quantisation code that pokes `weight.data`, `weight.grad` or iterates
`named_parameters()` sees live engine state.  A logical width the kernels are not instantiated for runs zero-padded to the
next one: its Parameters stay ordinary tensors, scattered into the handle before every pass and gathered back after a step.

A subclass supplies `cfg`, `_param_list()`, `_layer_fans()`, `_engine_width`, `_padded`, `_new_engine(H, w, row_begin,
row_end, device)` and, for `make decode`, `_new_render_engine(rows, cols, device, side)`: the inference-only handle from the
same `cfg`, a render call of which draws up to rows x cols samples (side: the whole picture's, for WaveletSiren), and which
`_load_render_engine(eng)` fills.  What else differs goes into the small hooks below.  Consumers (EngineAdam, train_epoch,
train_steps, Masking, KmeansQuant, decode) use the public names alone: `bound_engine`, `register_optimizer`, `mask_unsupported`,
the two callback lists, `state_is_live`, `adam_moments`, the hooks around the optimiser's device step, `download_grads`,
`set_engine_masks`, `engine_flat` and the two render hooks.  Which layout a model runs in (`_padded`) is read in this file only.
"""
import weakref
from typing import Optional

import torch
from torch import nn

from ..data import grid_vectors


class EngineBound(nn.Module):
    mask_unsupported = None        # the refusal setup_mask raises for a family the reference's Masking itself fails on
    # Two switches that exist only to keep, call for call and word for word, what each family did while it had its own copy
    # of this protocol (tests/golden/binding_trace.json pins the calls).  Neither is part of the design; both can go once a
    # change of behaviour is wanted: one sync before the optimisers are rebound serves every family, and a FourierNet
    # should refuse a CPU grid under its own name.
    _WHO = None                    # the name the device check refuses with (default: the class's; FourierNet: "Siren")
    _SYNC_PER_OPTIM = True         # a re-made handle syncs before EACH optimiser it rebinds (FeatherNet: once, in _carry_in)

    def __init__(self):
        super().__init__()
        # callbacks run right before every engine pass / right after every backward: the seam the reference
        # fills with per-Linear forward-pre and backward hooks (k-means quantisation, pipeline/quant/kmeans.py:39-55)
        self.pre_pass_callbacks = []
        self.post_backward_callbacks = []
        self._adam = ((0.9, 0.999), 1e-8)      # torch.optim.Adam defaults; EngineAdam overrides (conf/optim/*.yaml)
        self._padded = False                   # the subclass's constructor says (engine width != logical width)
        self._pad_index = None
        self._has_engine_mask = False
        self._engine = None
        self._engine_key = None
        self._grid_key = None
        self._target_key = None
        self._engine_optims = weakref.WeakSet()     # engine() rebinds these when it re-makes the handle
        self._split = None                     # a parallel.RowSplit: engine() then makes a handle of its rows alone

    # ---- what consumers use ---------------------------------------------------------------------
    split_unsupported = None       # the refusal set_row_split raises for a family whose handle has no row ranges

    @property
    def row_split(self):
        """the parallel.RowSplit this model is fitted under (train.pixel_split), None for an ordinary fit"""
        return self._split

    def set_row_split(self, split):
        """Fit this model on rows [split.row_begin, split.row_end) of a picture of split.full_height rows: engine(grid, img)
        takes the row range from here, so every consumer that asks for the handle meets the same one.  `grid` / `img` are
        then those rows (or the full-height grid); the step and evaluation harness reduces over the ranks (train_helper)."""
        if split is not None and self.split_unsupported:
            raise NotImplementedError(self.split_unsupported)
        self._split = split
    @property
    def bound_engine(self):
        """the live engine handle, None while unbound"""
        return self._engine

    def register_optimizer(self, optim):
        """`optim` (an EngineAdam on this model) is rebound to every handle engine() re-makes"""
        self._engine_optims.add(optim)

    @property
    def state_is_live(self) -> bool:
        """are the Parameters, their .grad and the Adam moments zero-copy views of the handle's vectors (a padded width: no)"""
        return not self._padded

    def adam_moments(self):
        """[(exp_avg, exp_avg_sq)] per parameter of `_param_list()`, as an optimiser holds them: live slices, else logical clones"""
        pairs = zip(self._state_slices("exp_avg"), self._state_slices("exp_avg_sq"))
        return [(m.clone(), v.clone()) if self._padded else (m, v) for m, v in pairs]

    def before_optimizer_step(self, take_moments):
        """The two hooks around an optimiser's device step; `take_moments(eng, again=False)` makes it hold adam_moments(), once
        per handle unless `again`.  Live state is bound before; a padded width gathers parameters and fresh clones after."""
        if not self._padded:
            take_moments(self._engine)

    def after_optimizer_step(self, take_moments):
        if self._padded:
            self.download_params()
            take_moments(self._engine, again=True)

    def set_scratch_format(self, fmt: int):
        """sf_config.scratch_format of the engine (0 auto / 8 / 12 / 16); a live engine of another format is rebuilt on
        the next pass: engine() carries the parameters, the Adam moments and step count (sf_get/set_adam_state) and the
        masks over to the new handle and rebinds every EngineAdam created on this model, so a switch in the middle of a
        fit neither resets the optimiser nor leaves `optimizer.state[p]` pointing at freed device memory."""
        self.cfg["scratch_format"] = int(fmt)

    def set_adam_hparams(self, betas, eps: float):
        """Adam betas / eps of the engine's fused optimiser kernel (sf_config); a live engine created with other
        values is rebuilt on the next pass, and its moments and step count are carried to the re-made handle."""
        self._adam = (tuple(betas), float(eps))

    # ---- the handle -----------------------------------------------------------------------------
    def _check_device(self, grid: torch.Tensor):
        if not grid.is_cuda:
            raise RuntimeError(f"{self._WHO or type(self).__name__} runs on the gfx950 engine only: move model, grid and "
                               "image to 'cuda'")

    def _engine_key_of(self, H: int, w: int, row_begin: int, row_end: int, device):
        return (H, w, row_begin, row_end, device, self._adam, self.cfg["scratch_format"])

    def _new_engine(self, H: int, w: int, row_begin: int, row_end: int, device: int):
        raise NotImplementedError

    def _carry_out(self, old):
        """what a re-made handle takes over from `old`: the Adam state, the masks, and what both must agree on"""
        m, v, st = old.get_adam_state()
        masks = old.view("masks").clone() if self._has_engine_mask else None
        return (m, v, st, masks, old.num_params, (old.height, old.width, old.row_begin, old.row_end))

    def _carry_in(self, new, carry):
        if carry is not None and carry[4] == new.num_params and carry[5] == (new.height, new.width, new.row_begin, new.row_end):
            # same fit on a re-created handle (another scratch format / Adam hyper-parameters): the optimiser goes along
            new.set_adam_state(carry[0], carry[1], carry[2])
            if carry[3] is not None:
                new.set_masks(carry[3])
        else:
            self._has_engine_mask = False

    def engine(self, grid: torch.Tensor, img: Optional[torch.Tensor] = None, row_begin: int = 0, row_end: int = 0,
               full_height: Optional[int] = None):
        """Engine bound to this model for `grid` (created on first use; re-made when the image size, the row range, the
        Adam hyper-parameters or the scratch format change)."""
        self._check_device(grid)
        h, w, _ = grid.shape
        split = self._split
        if split is not None and not (row_begin or row_end or full_height):
            row_begin, row_end, full_height = split.row_begin, split.row_end, split.full_height
        H = full_height or h
        key = self._engine_key_of(H, w, row_begin, row_end, grid.device.index)
        if self._engine is None or self._engine_key != key:
            carry = None
            if self._engine is not None:
                carry = self._carry_out(self._engine)
                self._unbind()
            self._engine = new = self._new_engine(H, w, row_begin, row_end, grid.device.index or 0)
            self._engine_key, self._grid_key, self._target_key = key, None, None
            self._carry_in(new, carry)
            for opt in list(self._engine_optims):
                if self._SYNC_PER_OPTIM and not self._padded:
                    self._sync_to_engine()
                opt.handle_changed()
        eng = self._engine
        gkey = (grid.data_ptr(), tuple(grid.shape))
        if self._grid_key != gkey:
            rows, cols = grid_vectors(grid)
            if full_height and full_height != h:
                # the handle indexes the row vector by absolute row: a grid of the split's rows alone brings the columns, the
                # split the rows of the whole picture
                full = None if split is None else split.row_coords
                if full is None or h != row_end - row_begin or full.numel() != full_height:
                    raise ValueError("pass the full-height grid in pixel-split mode")
                full = full.to(rows.device, rows.dtype)
                if not torch.equal(full[row_begin:row_end], rows):
                    raise ValueError(f"the grid does not hold rows [{row_begin}, {row_end}) of the split's row coordinates")
                rows = full
            eng.set_coords(rows.float(), cols.float())
            self._grid_key = gkey
        if img is not None:
            tkey = (img.data_ptr(), tuple(img.shape), img._version)
            if self._target_key != tkey:
                eng.set_target(img.contiguous().float())
                self._target_key = tkey
        for cb in list(self.pre_pass_callbacks):
            cb()
        self._sync_to_engine()
        return eng

    def _bind_params(self, eng):
        """(Re)bind every Parameter (and .grad) to its slice of the handle's flat params / grads views.  Code that
        REPLACED `weight.data` (e.g. `weight.data = weight.data * mask`) is detected by pointer and copied in."""
        flat, grads = eng.view("params"), eng.view("grads")
        off = 0
        for p in self._param_list():
            n = p.numel()
            dst = flat[off:off + n].view(p.shape)
            if p.data.data_ptr() != dst.data_ptr():
                dst.copy_(p.data.to(dst.dtype))
                p.data = dst
            g = grads[off:off + n].view(p.shape)
            if p.grad is None or p.grad.data_ptr() != g.data_ptr():
                p.grad = g
            off += n

    def _load_render_engine(self, eng):
        """put this model's state into the handle its _new_render_engine made (a family with more than flat parameters adds it)"""
        eng.set_params(self._flat_for(eng.num_params, eng.device))

    def _flat_for(self, num_params: int, device) -> torch.Tensor:
        """`_param_list()` as the flat vector of a handle with num_params slots on `device`, zero-padded by engine_flat"""
        logical = torch.cat([p.data.reshape(-1).float() for p in self._param_list()])
        if self._padded:
            return self.engine_flat(logical, num_params, device)
        if logical.numel() != num_params:
            raise ValueError(f"the state dict holds {logical.numel()} parameters, the engine handle {num_params}")
        return logical.contiguous().to(device)

    def _sync_to_engine(self):
        """Hand the handle the current parameters.  Padded widths: they are scattered into the engine every pass."""
        eng = self._engine
        if self._padded:
            eng.set_params(self._flat_for(eng.num_params, eng.device))
            return
        self._bind_params(eng)
        eng.params_changed()   # in-place edits through the views are invisible to the engine: always refresh

    def _unbind(self):
        for p in self._param_list():
            p.data = p.data.clone()
            p.grad = None if not self._padded else p.grad
        self._engine.close()
        self._engine = None

    def half(self):
        """model.half() of the reference's save path (compress.py:246-250): detaches from the engine."""
        if self._engine is not None:
            self._unbind()
        return super().half()

    def forward(self, grid: torch.Tensor) -> torch.Tensor:
        """[H, W, 2] grid -> [H, W, output_size] prediction (the reference's call signature)."""
        pred, _ = self.engine(grid).forward(want_pred=True, want_sse=False)
        return pred

    # ---- padded widths --------------------------------------------------------------------------
    def _layer_fans(self):
        """(fan_in, fan_out, fan_in is padded, fan_out is padded) of every layer in flat order, logical sizes: all that
        _padded_index needs to know of a network (the hidden side of a layer runs at the engine width, its ends do not)"""
        raise NotImplementedError

    def _padded_index(self, device):
        """flat index of every logical parameter element inside the engine's (wider) flat layout"""
        if self._pad_index is None or self._pad_index.device != device:
            wp = self._engine_width
            idx, off = [], 0
            for fin, fout, pad_in, pad_out in self._layer_fans():
                fin_p, fout_p = (wp if pad_in else fin), (wp if pad_out else fout)
                r = torch.arange(fout, device=device)[:, None] * fin_p + torch.arange(fin, device=device)[None, :]
                idx.append((off + r).reshape(-1))
                off += fin_p * fout_p
                idx.append(off + torch.arange(fout, device=device))
                off += fout_p
            self._pad_index = torch.cat(idx)
        return self._pad_index

    def engine_flat(self, logical: torch.Tensor, num_params: int, device) -> torch.Tensor:
        """A padded model's logical flat vector (parameters, masks) scattered into a handle's layout of `num_params`
        slots on `device`: zeros in the padding.  The one logical -> engine-flat scatter."""
        flat = torch.zeros(num_params, device=device)
        flat[self._padded_index(device)] = logical.to(device).float()
        return flat

    def _state_slices(self, which: str):
        """an engine state vector ('params' | 'grads' | 'exp_avg' | ...) as one tensor per parameter of `_param_list()`:
        views of it when the state is live, slices of one logical gather of it when padded"""
        flat = self._engine.view(which)
        if self._padded:
            flat = flat[self._padded_index(self._engine.device)]
        out, off = [], 0
        for p in self._param_list():
            out.append(flat[off:off + p.numel()].view(p.shape))
            off += p.numel()
        return out

    def download_grads(self):
        """after a backward: make `.grad` current (bound views are; a padded width gathers its logical slices)"""
        if self._padded:
            for p, g in zip(self._param_list(), self._state_slices("grads")):
                p.grad = g.clone()

    def download_params(self):
        if self._padded:
            for p, v in zip(self._param_list(), self._state_slices("params")):
                p.data.copy_(v)

    def set_engine_masks(self, flat_logical: torch.Tensor):
        """0/1 mask per logical parameter element -> engine (scattered into the wider layout when padded)."""
        eng = self._engine
        self._has_engine_mask = True
        eng.set_masks(self.engine_flat(flat_logical, eng.num_params, eng.device) if self._padded else flat_logical.contiguous())

    # ---- copies ---------------------------------------------------------------------------------
    def _ctor_args(self) -> dict:
        """Keyword arguments that rebuild this model, for type(self): `cfg` holds every family's.  This leans on two things:
        every constructor takes **kwargs, which swallows the keys of cfg that are not arguments (FourierNet's n_linear and
        scratch_format), and cfg's hidden_size is already the Small_Dense one, so small_dense_density stays at its default.
        A subclass whose constructor takes other arguments overrides this hook (the copy is of the subclass's type)."""
        return dict(self.cfg)

    def _copy_extras(self, new):
        """what a deep copy takes along besides `_param_list()` (called under no_grad)"""

    def __deepcopy__(self, memo):
        new = type(self)(**self._ctor_args())
        new.to(next(self.parameters()).device)
        new._adam = self._adam
        new._split = self._split               # (a copy is fitted on the same rows: the quantise phase)
        with torch.no_grad():
            for a, b in zip(new._param_list(), self._param_list()):
                a.copy_(b)
            self._copy_extras(new)
        new.train(self.training)
        return new
