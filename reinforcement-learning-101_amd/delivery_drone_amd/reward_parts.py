"""The notebooks' ``rewards`` list from a batched evaluation.

The notebooks' ``evaluate_policy`` returns ``rewards``: one ``calc_reward``
dict per frame of the episode, which ``plot_accumulated_rewards`` accumulates
per key.  :meth:`VecDroneEnv.evaluate_policy` with ``components=True,
per_frame=True`` keeps the same values for every lane as ``[max_steps, N]``
tensors; :func:`notebook_rewards` reads one lane back in the notebook's format.
"""
from __future__ import annotations

__all__ = ["notebook_rewards"]


def notebook_rewards(result: dict, lane: int) -> list:
    """The list of per-frame ``calc_reward`` dicts of lane ``lane``, as long as
    that lane's ``steps``, from the result of ``evaluate_policy(...,
    components=True, per_frame=True)``.  Each dict has the notebook's keys in
    its order (``total`` last) with Python floats, so
    ``plot_accumulated_rewards({"rewards": notebook_rewards(res, lane)})`` of
    the notebooks runs on it unchanged."""
    if "rewards" not in result:
        raise ValueError("notebook_rewards needs evaluate_policy(..., components=True, per_frame=True)")
    steps = int(result["steps"][lane])
    columns = {name: frames[:steps, lane].tolist() for name, frames in result["rewards"].items()}
    return [{name: col[k] for name, col in columns.items()} for k in range(steps)]
