"""Flat gradient / optimiser storage for one parameter list: every ``.grad`` is a view into
one bucket, and -- when the optimiser is a plain ``torch.optim.Adam`` or a plain
``torch.optim.RMSprop`` over exactly these parameters -- the parameters and their moments
(``exp_avg`` / ``exp_avg_sq``, or ``square_avg``) become views into flat buffers, so
``clip_grad_norm_`` + ``optim.step()`` (ppo.py:143-151, a2c.py:139-147) run as ONE HIP pass
(``tsrl_clip_adam`` / ``tsrl_clip_rmsprop``, csrc/optim.hip) whose learning rate is a device
word.  Both properties
make a whole epoch of minibatches capturable as one HIP graph: no host-side optimiser logic,
no allocation, no synchronisation.

``optim.state[p]`` entries are views too, so ``optim.state_dict()`` and torch's own
``optim.step()`` work on the same storage; after ``optim.load_state_dict()`` the next
``adam_bound`` check copies the loaded moments and step counts into the flat storage.

Used by the fused Gaussian MLP (policy/fused_mlp.py, which adds its kernels' pointers) and by
the Categorical learn path of A2CPolicy / PPOPolicy (any torch actor / critic networks).  The
method names keep "adam" (bind_adam, adam_bound, clip_adam): they serve either optimiser.
"""
from typing import Optional

import torch

from tianshou_amd import _C


def _slot(flat: torch.Tensor, o: int, p: torch.Tensor) -> torch.Tensor:
    """The numel(p) words of ``flat`` from offset o viewed with p's shape AND memory format
    (a channels_last conv weight stays channels_last: MIOpen would otherwise copy an NCHW
    weight to the input's format on every convolution, and autograd would accumulate its
    channels_last gradients into NCHW slots with a strided add)."""
    k = p.numel()
    if p.is_contiguous():
        return flat[o:o + k].view_as(p)
    stride = torch.empty_like(p, memory_format=torch.preserve_format).stride()
    return flat.as_strided(p.shape, stride, flat.storage_offset() + o)


class FlatAdam:
    # extra f32 words after the flat gradients in the bucket (data-parallel loss sums ride
    # in the same all-reduce as the gradients)
    BUCKET_TAIL = 0

    def __init__(self, params) -> None:
        self.params = [p for p in params]
        self._flat = None
        self._bucket = None
        self._views = []
        self._adam = None  # flat parameter / moment storage of bind_adam (Adam or RMSprop)

    # -- gradient storage -----------------------------------------------------------------------
    def bind_grads(self) -> None:
        """Point every parameter's .grad at a slice of one flat buffer (kept across
        minibatches; re-bound if the optimiser or user replaced a .grad)."""
        dev = self.params[0].device
        if self._flat is not None and all(
                p.grad is not None and p.grad.data_ptr() == v.data_ptr()
                for p, v in zip(self.params, self._views)):
            return
        n = sum(p.numel() for p in self.params)
        self._bucket = torch.zeros(n + self.BUCKET_TAIL, dtype=torch.float32, device=dev)
        self._flat = self._bucket[:n]
        self._views = []
        o = 0
        for p in self.params:
            v = _slot(self._flat, o, p)
            p.grad = v
            self._views.append(v)
            o += p.numel()
        self._grads_bound()

    def _grads_bound(self) -> None:
        """Hook: the gradient addresses changed."""

    @property
    def flat_grad(self) -> Optional[torch.Tensor]:
        return self._flat

    def zero_grad(self) -> None:
        """optim.zero_grad() for views that must keep their addresses: autograd then
        accumulates into the flat bucket in place."""
        self.bind_grads()
        self._flat.zero_()

    def release_grads(self) -> None:
        """zero_grad() for an eager backward followed by gather_grads(): the slots stay bound
        (their addresses are the ones the optimiser pass and the collectives use), every .grad
        is set to None, and autograd then hands each parameter its gradient tensor as it is
        instead of adding it into a zero-filled slot -- the fill and one add per parameter
        saved (round 6; 12 of each per config-5 minibatch)."""
        self.bind_grads()
        for p, v in zip(self.params, self._views):
            p.grad = None
            # a custom backward that can write a gradient in place (net_atari's Flatten +
            # Linear) finds its slot here, writes it and makes it the .grad
            p._tsrl_flat_slot = v

    def gather_grads(self) -> None:
        """After a backward that began with release_grads(): every parameter's gradient copied
        into its slot in one multi-tensor pass (a slot whose parameter received no gradient is
        zeroed, as zero_grad() would have left it) and every .grad pointed back at its slot."""
        dst, src = [], []
        for p, v in zip(self.params, self._views):
            p.__dict__.pop("_tsrl_flat_slot", None)
            g = p.grad
            if g is None:
                v.zero_()
            elif g.data_ptr() != v.data_ptr():
                if g.shape != v.shape or g.dtype != v.dtype:
                    raise RuntimeError("FlatAdam.gather_grads: a gradient does not match its "
                                       f"parameter ({tuple(g.shape)} {g.dtype} vs "
                                       f"{tuple(v.shape)} {v.dtype})")
                dst.append(v)
                src.append(g)
            p.grad = v
        if dst:
            torch._foreach_copy_(dst, src)

    # -- clip_grad_norm_ + Adam as one HIP pass ---------------------------------------------------
    @staticmethod
    def _plain_kind(optim, params) -> Optional[str]:
        """"adam" / "rmsprop" when ``optim`` is the plain form of that optimiser over exactly
        ``params`` in one group (the update the HIP pass computes), else None."""
        if len(optim.param_groups) != 1:
            return None
        g = optim.param_groups[0]
        if g.get("weight_decay", 0) != 0 or g.get("maximize") or g.get("differentiable") or \
                isinstance(g["lr"], torch.Tensor):
            return None
        if isinstance(optim, torch.optim.Adam):
            if g.get("amsgrad"):
                return None
            kind = "adam"
        elif isinstance(optim, torch.optim.RMSprop):
            if g.get("momentum", 0) != 0 or g.get("centered"):
                return None
            kind = "rmsprop"
        else:
            return None
        if len(g["params"]) != len(params) or \
                not all(a is b for a, b in zip(g["params"], params)):
            return None
        return kind

    # optim.state[p] keys of each kind's moments, in the order of the flat buffers
    MOMENTS = {"adam": ("exp_avg", "exp_avg_sq"), "rmsprop": ("square_avg",)}

    def adam_bound(self, optim) -> bool:
        """The flat storage serves ``optim``: same optimiser, parameters still views into the
        flat buffer.  If ``optim.state`` no longer holds the flat views (``load_state_dict``
        installs new exp_avg / exp_avg_sq / step tensors), the loaded moments and step counts
        are copied into the flat storage and the views re-installed, so a restored state is
        what the next clip_adam pass continues from."""
        st = self._adam
        if st is None or st["optim"] is not optim or not all(
                p.data_ptr() == v.data_ptr() for p, v in zip(self.params, st["pviews"])):
            return False
        if not self._state_is_flat(optim):
            if not self._uniform_steps(optim, self.params):
                # a partial / mixed state dict: torch's Adam keeps one step count per
                # parameter, the flat pass one for all -- hand the step back to torch
                self._adam = None
                return False
            self._rebind_state(optim)
        return True

    @staticmethod
    def _uniform_steps(optim, params) -> bool:
        """Every parameter's optimiser step count is the same (a parameter without state counts
        0).  clip_adam applies one bias correction to all parameters, so only then is it the
        update torch's Adam would make."""
        ks = set()
        for p in params:
            s = optim.state.get(p, {})
            ks.add(float(s["step"]) if "step" in s else 0.0)
        return len(ks) <= 1

    def _state_is_flat(self, optim) -> bool:
        st = self._adam
        for i, p in enumerate(self.params):
            s = optim.state.get(p)
            if s is None:
                return False
            for name, views in zip(st["names"], st["views"]):
                m = s.get(name)
                if not isinstance(m, torch.Tensor) or m.data_ptr() != views[i].data_ptr():
                    return False
            k = s.get("step")
            if not isinstance(k, torch.Tensor) or k.data_ptr() != st["steps"][i].data_ptr():
                return False
        return True

    def _rebind_state(self, optim) -> None:
        """Copy whatever ``optim.state`` now holds into the flat moments / step counts (zeros
        for a parameter without state) and point ``optim.state`` back at the flat views."""
        st = self._adam
        for i, p in enumerate(self.params):
            s = optim.state.get(p, {})
            if st["names"][0] in s:
                for name, views in zip(st["names"], st["views"]):
                    views[i].copy_(s[name])
                st["steps"][i].copy_(torch.as_tensor(s["step"], dtype=torch.float32))
            else:
                for views in st["views"]:
                    views[i].zero_()
                st["steps"][i].zero_()
            optim.state[p] = {"step": st["steps"][i],
                              **{name: views[i] for name, views in zip(st["names"],
                                                                       st["views"])}}
        st["lr_host"] = None  # load_state_dict may also have changed the param-group lr

    def bind_adam(self, optim) -> bool:
        """Move every parameter and its moments into flat buffers (parameter .data and
        ``optim.state[p]`` become views) when ``optim`` is a plain Adam or a plain RMSprop
        over exactly these parameters; then ``clip_adam`` replaces clip_grad_norm_ +
        optim.step()."""
        if self.adam_bound(optim):
            return True
        kind = self._plain_kind(optim, self.params)
        if kind is None or not self._uniform_steps(optim, self.params):
            self._adam = None
            return False
        dev = self.params[0].device
        n = sum(p.numel() for p in self.params)
        names = self.MOMENTS[kind]
        flat_p = torch.empty(n, dtype=torch.float32, device=dev)
        flats = [torch.zeros(n, dtype=torch.float32, device=dev) for _ in names]
        steps = torch.zeros(len(self.params), dtype=torch.float32, device=dev)
        pviews, views = [], [[] for _ in names]
        o = 0
        for i, p in enumerate(self.params):
            k = p.numel()
            pv = _slot(flat_p, o, p)
            mv = [_slot(f, o, p) for f in flats]
            pv.copy_(p.detach())
            st = optim.state.get(p, {})
            if names[0] in st:
                for name, v in zip(names, mv):
                    v.copy_(st[name])
                steps[i] = float(st["step"])
            with torch.no_grad():
                p.data = pv
            optim.state[p] = {"step": steps[i], **dict(zip(names, mv))}
            pviews.append(p.data)
            for vs, v in zip(views, mv):
                vs.append(v)
            o += k
        self._adam = dict(optim=optim, kind=kind, names=names, p=flat_p, flats=flats,
                          steps=steps, pviews=pviews, views=views,
                          ticket=torch.zeros(3, dtype=torch.int32, device=dev),
                          partials=torch.zeros(
                              max(int(_C.lib().tsrl_clip_adam_partials(n)), 1),
                              dtype=torch.float64, device=dev),
                          norm=torch.zeros(2, dtype=torch.float32, device=dev),
                          lr=torch.zeros(1, dtype=torch.float32, device=dev))
        self._flat = None  # parameter addresses moved: bind_grads re-derives every pointer
        self.bind_grads()
        return True

    @property
    def flat_param(self) -> Optional[torch.Tensor]:
        """The flat parameter buffer of bind_adam (None while unbound): DQNPolicy lays its
        target network out the same way, so a hard sync is one copy."""
        return None if self._adam is None else self._adam["p"]

    def flat_offset(self, t: torch.Tensor) -> int:
        """Element offset of parameter storage ``t`` inside the flat parameter buffer."""
        return (t.data_ptr() - self._adam["p"].data_ptr()) // 4

    def set_lr(self) -> None:
        """Publish the optimiser's current lr to the device word the Adam kernel reads (one
        tiny fill per epoch; captured learn graphs then follow an lr_scheduler without being
        re-captured)."""
        st = self._adam
        lr = float(st["optim"].param_groups[0]["lr"])
        if st.get("lr_host") != lr:
            st["lr"].fill_(lr)
            st["lr_host"] = lr

    def clip_adam(self, max_norm: Optional[float], scale_grads: bool = True,
                  split=None) -> None:
        """clip_grad_norm_(max_norm) (when given) + the bound optimiser's step() (Adam or
        RMSprop, by the kind bind_adam found) over the flat buffers; the
        learning rate comes from the device word of set_lr().  ``scale_grads=False`` skips
        the in-place clipping of .grad (only the last step of a learn() needs it: every
        minibatch overwrites the gradients); ``split`` (a _C.W1Split) re-splits first-layer
        weights into bf16x6 planes in the same pass."""
        st = self._adam
        g = st["optim"].param_groups[0]
        if st.get("lr_host") is None:
            self.set_lr()
        head = (_C.ptr(st["p"]), _C.ptr(self._flat), *(_C.ptr(f) for f in st["flats"]),
                st["p"].numel(), _C.ptr(st["steps"]), st["steps"].numel(), float(g["lr"]))
        tail = (float(g["eps"]), float(max_norm) if max_norm else 0.0, _C.ptr(st["partials"]),
                _C.ptr(st["norm"]), _C.ptr(st["ticket"]), _C.ptr(st["lr"]), split,
                int(bool(scale_grads)), _C.stream_ptr(st["p"].device))
        if st["kind"] == "adam":
            b1, b2 = g["betas"]
            _C.check(_C.lib().tsrl_clip_adam(*head, float(b1), float(b2), *tail),
                     "tsrl_clip_adam")
        else:
            _C.check(_C.lib().tsrl_clip_rmsprop(*head, float(g["alpha"]), *tail),
                     "tsrl_clip_rmsprop")

    def check_handoff(self) -> None:
        """Raise if any clip_adam launch since the last check timed out waiting for the slice
        norms of the other workgroups (tsrl_clip_adam's sticky ticket[2]): its step used a
        NaN clip coefficient in some slices only, so the parameters are invalid.  One 4-byte
        read, after learn() has read its loss terms back anyway."""
        st = self._adam
        if st is not None and int(st["ticket"][2].item()) != 0:
            st["ticket"][2].zero_()
            raise RuntimeError("tsrl_clip_adam: the in-kernel gradient-norm hand-off timed out "
                               "(workgroups not co-resident); this learn()'s parameters are "
                               "invalid")
