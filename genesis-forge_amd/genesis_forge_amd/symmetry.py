"""
Mirror symmetry for the PPO update (rsl_rl's ``symmetry_cfg``): the left/right mirror of a legged robot as a signed permutation of
every tensor kind the learner sees.

:class:`MirrorSymmetry` holds three tables — policy observations, critic observations, actions::

    mirror(x)[n, j] = sign[j] * x[n, perm[j]]

validated on the host when it is built (a permutation, signs ±1, an involution: mirroring twice is the identity) and uploaded once
per device as int32 / float32.  Those device tables are the only ones ``gf_mirror_rows`` / ``gf_mirror_loss`` ever see — the kernels
trust them (include/gf_step.h).  The object is also rsl_rl's ``data_augmentation_func``: called with rsl_rl's signature it returns the
batch followed by its mirror, in plain torch — so the same object drives ``learner.PPO`` on the HIP path, on the CPU oracle backend,
and real rsl_rl.

An observation here is a concatenation of manager items, possibly with history: :meth:`MirrorSymmetry.from_items` builds the
full-width tables from per-item ones, :meth:`MirrorSymmetry.repeat_frames` repeats a one-frame table over ``history_len`` frames.
"""
from __future__ import annotations

from typing import Dict, Mapping, Optional, Sequence, Tuple

import torch

_KINDS = ("policy", "critic", "actions")


def _table(perm, sign, name: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """``perm`` / ``sign`` as validated CPU tensors (int64 / float32); ``ValueError`` naming the table otherwise."""
    try:
        p = torch.as_tensor(perm).detach().cpu()
        s = torch.as_tensor(sign).detach().cpu()
    except Exception as e:   # (a ragged list, a string)
        raise ValueError(f"MirrorSymmetry: {name}_perm / {name}_sign must be flat sequences of numbers ({e})") from None
    if p.dim() != 1 or p.numel() < 1:
        raise ValueError(f"MirrorSymmetry: {name}_perm must be a flat, non-empty sequence")
    if p.is_floating_point() or p.dtype == torch.bool:
        if p.dtype == torch.bool or not bool((p == p.round()).all()):
            raise ValueError(f"MirrorSymmetry: {name}_perm must hold integers")
    p = p.to(torch.int64)
    w = int(p.numel())
    if s.dim() != 1 or int(s.numel()) != w:
        raise ValueError(f"MirrorSymmetry: {name}_sign has {tuple(s.shape)} entries, {name}_perm {w}")
    s = s.to(torch.float32)
    if not torch.equal(torch.sort(p).values, torch.arange(w)):
        raise ValueError(f"MirrorSymmetry: {name}_perm is not a permutation of 0 … {w - 1}")
    if not bool(((s == 1.0) | (s == -1.0)).all()):
        raise ValueError(f"MirrorSymmetry: {name}_sign must be +1 or -1 everywhere")
    if not torch.equal(p[p], torch.arange(w)):
        raise ValueError(f"MirrorSymmetry: {name}_perm is not an involution (perm[perm[j]] != j): mirroring twice must give the input back")
    if not bool((s * s[p] == 1.0).all()):
        raise ValueError(f"MirrorSymmetry: {name}_sign is not an involution (sign[j] * sign[perm[j]] != 1): mirroring twice must give the input back")
    return p, s


def _item_widths(source) -> Tuple[list, int]:
    """``[(item name, width)]`` of one frame and the history length of an ObservationManager, a ``{name: width}`` mapping or a
    sequence of ``(name, width)`` pairs (history 1)."""
    plan = getattr(source, "_plan", None)
    if plan is not None or hasattr(source, "observation_space"):
        if not plan:
            raise ValueError("MirrorSymmetry.from_items: the ObservationManager is not built yet (its item widths are not known)")
        return [(name, int(w)) for name, _cfg, _src, w in plan], int(getattr(source, "_history_len", 1))
    pairs = list(source.items()) if isinstance(source, Mapping) else list(source)
    try:
        out = [(str(name), int(w)) for name, w in pairs]
    except Exception:
        raise ValueError("MirrorSymmetry.from_items: expected an ObservationManager, a {name: width} mapping or (name, width) pairs") from None
    if not out or any(w < 1 for _n, w in out):
        raise ValueError("MirrorSymmetry.from_items: every item needs a width >= 1")
    return out, 1


class MirrorSymmetry:
    """One mirror of the robot as signed permutations of the policy observation, the critic observation (``None``: the policy
    tables) and the action vector.  ``ValueError`` (naming the table) unless each ``perm`` is a permutation of ``0 … W-1``, each
    ``sign`` is ±1 and the map is an involution.

    ``sym(obs=None, actions=None, env=None, obs_type="policy")`` is rsl_rl's ``data_augmentation_func``: ``(cat([obs, mirror(obs)]),
    cat([actions, mirror(actions)]))`` with ``None`` passed through; ``obs_type="critic"`` uses the critic tables."""

    num_aug = 2   # the batch and one mirrored copy

    def __init__(self, obs_perm, obs_sign, act_perm, act_sign, critic_obs_perm=None, critic_obs_sign=None):
        if (critic_obs_perm is None) != (critic_obs_sign is None):
            raise ValueError("MirrorSymmetry: critic_obs_perm and critic_obs_sign come together")
        self._host: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {"policy": _table(obs_perm, obs_sign, "obs"), "actions": _table(act_perm, act_sign, "act")}
        self._host["critic"] = self._host["policy"] if critic_obs_perm is None else _table(critic_obs_perm, critic_obs_sign, "critic_obs")
        self._dev: Dict[Tuple[str, torch.device], Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = {}

    # -- widths, tables ------------------------------------------------------------------------------------------------------------
    @property
    def obs_width(self) -> int:
        return int(self._host["policy"][0].numel())

    @property
    def critic_obs_width(self) -> int:
        return int(self._host["critic"][0].numel())

    @property
    def num_actions(self) -> int:
        return int(self._host["actions"][0].numel())

    def host_tables(self, kind: str = "policy") -> Tuple[torch.Tensor, torch.Tensor]:
        """``(perm int64, sign float32)`` of ``kind`` (``"policy"``, ``"critic"`` or ``"actions"``) on the CPU, as validated (clones)."""
        p, s = self._host[self._kind(kind)]
        return p.clone(), s.clone()

    def tables(self, kind: str, device) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(perm int32, sign float32)`` of ``kind`` on ``device`` — uploaded on first use, the same tensors ever after: what the
        kernels read."""
        t = self._tables(kind, device)
        return t[0], t[1]

    def _tables(self, kind: str, device):
        key = (self._kind(kind), torch.device(device))
        t = self._dev.get(key)
        if t is None:
            p, s = self._host[key[0]]
            t = self._dev[key] = (p.to(torch.int32).to(key[1]), s.to(key[1]), p.to(key[1]))   # (int32 for the kernels, int64 for torch indexing)
        return t

    @staticmethod
    def _kind(kind: str) -> str:
        if kind not in _KINDS:
            raise ValueError(f"MirrorSymmetry: unknown table {kind!r} (one of {_KINDS})")
        return kind

    def mirror(self, x: torch.Tensor, kind: str = "policy") -> torch.Tensor:
        """``sign * x[..., perm]`` in plain torch (a new tensor)."""
        _p32, s, p = self._tables(kind, x.device)
        if x.shape[-1] != p.numel():
            raise ValueError(f"MirrorSymmetry: the {kind} table is {p.numel()} wide, the tensor {x.shape[-1]}")
        return s.to(x.dtype) * x[..., p]

    def __call__(self, obs=None, actions=None, env=None, obs_type: str = "policy"):
        o = None if obs is None else torch.cat([obs, self.mirror(obs, "critic" if obs_type == "critic" else "policy")], dim=0)
        a = None if actions is None else torch.cat([actions, self.mirror(actions, "actions")], dim=0)
        return o, a

    # -- tables from the pieces of an observation ------------------------------------------------------------------------------------
    @staticmethod
    def repeat_frames(perm, sign, history_len: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The table of a ``history_len``-frame observation from the table of one frame.  An ObservationManager keeps its history as
        ``history_len`` whole frames side by side (newest first — ``RolloutStorage`` and every output mode agree), and a mirror acts on
        each frame alone: frame ``h`` of the result is the one-frame table shifted by ``h`` frame widths, whatever the frame order."""
        p, s = _table(perm, sign, "frame")
        H = int(history_len)
        if H < 1:
            raise ValueError("MirrorSymmetry.repeat_frames: history_len must be >= 1")
        w = int(p.numel())
        return torch.cat([p + h * w for h in range(H)]), s.repeat(H)

    @staticmethod
    def item_tables(source, items: Mapping[str, tuple], history_len: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Full-width ``(perm, sign)`` of an observation from per-item tables.  ``source``: a built ObservationManager (its items,
        widths and ``history_len`` are read from it), a ``{item name: width}`` mapping or ``(name, width)`` pairs in column order — or a
        sequence of those for an observation group of several managers side by side.  ``items``: ``{item name: (perm, sign)}``, indices
        relative to the item; an item that is not named is mirrored onto itself (identity).  ``history_len`` overrides the manager's.
        ``ValueError`` for a name the observation does not have and for a table of another width than its item."""
        pairs = lambda x: isinstance(x, (list, tuple)) and len(x) == 2 and isinstance(x[0], str)
        group = isinstance(source, (list, tuple)) and len(source) > 0 and not all(pairs(x) for x in source)
        members = [_item_widths(m) for m in (source if group else [source])]
        names = {n for widths, _H in members for n, _w in widths}
        unknown = sorted(k for k in items if k not in names)
        if unknown:
            raise ValueError(f"MirrorSymmetry.from_items: the observation has no item {unknown} (items: {sorted(names)})")
        out_p, out_s, offs = [], [], 0
        for widths, H in members:   # (a group: its members side by side, each with its own history)
            perms, signs, col = [], [], 0
            for name, w in widths:
                if name in items:
                    p, s = _table(items[name][0], items[name][1], f"item '{name}' ")
                    if int(p.numel()) != w:
                        raise ValueError(f"MirrorSymmetry.from_items: the table of item '{name}' is {int(p.numel())} wide, the item {w}")
                else:
                    p, s = torch.arange(w), torch.ones(w)
                perms.append(p + col)
                signs.append(s)
                col += w
            p, s = MirrorSymmetry.repeat_frames(torch.cat(perms), torch.cat(signs), H if history_len is None else int(history_len))
            out_p.append(p + offs)
            out_s.append(s)
            offs += int(p.numel())
        return torch.cat(out_p), torch.cat(out_s)

    @classmethod
    def from_items(cls, obs, obs_items: Mapping[str, tuple], act_perm, act_sign, critic_obs=None, critic_items: Optional[Mapping[str, tuple]] = None,
                   history_len: Optional[int] = None) -> "MirrorSymmetry":
        """A :class:`MirrorSymmetry` whose observation tables are built by :meth:`item_tables` — ``obs`` / ``critic_obs`` as its
        ``source`` (``critic_obs=None``: the critic reads the policy observation), ``critic_items=None``: ``obs_items``."""
        p, s = cls.item_tables(obs, obs_items, history_len)
        if critic_obs is None:
            return cls(p, s, act_perm, act_sign)
        cp, cs = cls.item_tables(critic_obs, obs_items if critic_items is None else critic_items, history_len)
        return cls(p, s, act_perm, act_sign, cp, cs)
