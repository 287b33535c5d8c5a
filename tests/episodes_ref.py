"""NumPy restatement of the every-episode training batch
(``delivery_drone_amd.ppo_episodes_batch`` / ``reinforce_episodes_batch``,
csrc/train_batch_episodes.hip): the rule that cuts a [T][N] rollout into
episodes from ``done`` and ``done_before`` alone, and the per-episode
arithmetic, which is ``train_batch_ref``'s (``gae_flat``, ``returns_flat``,
``normalize``) called once per episode.  ``test_train_batch_episodes_cpu.py``
pins it to the notebooks' own results (tests/golden/train_batch_episodes/); the
GPU tests compare the kernels with it."""
import numpy as np

import train_batch_ref as ref

F32 = np.float32


def kept_frames(done, done_before=None):
    """bool [T][N]: frame t of lane i is a candidate row unless the frame
    before it was done (done[t-1][i], or done_before[i] for t == 0)."""
    done = np.asarray(done) != 0
    T, n = done.shape
    before = np.zeros(n, dtype=bool) if done_before is None else np.asarray(done_before) != 0
    prev = np.concatenate([before[None, :], done[:-1]], axis=0) if T else done
    return ~prev


def layout(done, done_before=None, drop_open=False):
    """The seven layout arrays and the row map of done [T][N]:
    lane_episode / lane_row int64 [N+1], ep_lane / ep_start / ep_length int32
    [E], ep_ended uint8 [E], ep_offset int64 [E+1]; row_t / row_lane [M]: the
    frame and lane of every row."""
    done = np.asarray(done) != 0
    T, n = done.shape
    kept = kept_frames(done, done_before)
    lane_episode, lane_row = [0], [0]
    ep_lane, ep_start, ep_length, ep_ended, row_t, row_lane = [], [], [], [], [], []
    for i in range(n):
        run = []
        for t in range(T):
            if not kept[t, i]:
                assert not run  # a dropped frame follows a done, which closed the episode
                continue
            run.append(t)
            last = t == T - 1
            if done[t, i] or last:
                ended = bool(done[t, i])
                if ended or not drop_open:
                    assert run == list(range(run[0], run[0] + len(run)))
                    ep_lane.append(i)
                    ep_start.append(run[0])
                    ep_length.append(len(run))
                    ep_ended.append(ended)
                    row_t.extend(run)
                    row_lane.extend([i] * len(run))
                run = []
        lane_episode.append(len(ep_lane))
        lane_row.append(len(row_t))
    ep_length = np.asarray(ep_length, dtype=np.int32)
    ep_offset = np.zeros(len(ep_length) + 1, dtype=np.int64)
    np.cumsum(ep_length, out=ep_offset[1:])
    return dict(lane_episode=np.asarray(lane_episode, dtype=np.int64), lane_row=np.asarray(lane_row, dtype=np.int64),
                ep_lane=np.asarray(ep_lane, dtype=np.int32), ep_start=np.asarray(ep_start, dtype=np.int32),
                ep_length=ep_length, ep_ended=np.asarray(ep_ended, dtype=np.uint8), ep_offset=ep_offset,
                row_t=np.asarray(row_t, dtype=np.int64), row_lane=np.asarray(row_lane, dtype=np.int64))


LAYOUT_ARRAYS = ("lane_episode", "lane_row", "ep_lane", "ep_start", "ep_length", "ep_ended", "ep_offset")


def gather(x, lay):
    """The rows of x [T][N](...) in batch order."""
    return np.asarray(x)[lay["row_t"], lay["row_lane"]]


def _episodes(lay):
    for e in range(len(lay["ep_lane"])):
        yield (e, int(lay["ep_lane"][e]), int(lay["ep_start"][e]), int(lay["ep_length"][e]), bool(lay["ep_ended"][e]),
               int(lay["ep_offset"][e]))


def gae_flat(reward, values, lay, bootstrap=None, gamma=0.99, lam=0.95):
    """(advantages, returns) float32 [M] from values float32 [M] (batch
    order): train_batch_ref.gae_flat on each episode by itself."""
    reward = np.asarray(reward)
    values = np.asarray(values, dtype=F32)
    M = int(lay["ep_offset"][-1])
    adv, ret = np.zeros(M, dtype=F32), np.zeros(M, dtype=F32)
    for e, lane, start, ln, ended, off in _episodes(lay):
        a, r = ref.gae_flat(reward[start:start + ln, lane:lane + 1], values[off:off + ln], [ln], [0, ln], [ended],
                            None if bootstrap is None else [bootstrap[lane]], gamma, lam)
        adv[off:off + ln], ret[off:off + ln] = a, r
    return adv, ret


def returns_flat(reward, lay, gamma=0.99):
    reward = np.asarray(reward)
    out = np.zeros(int(lay["ep_offset"][-1]), dtype=F32)
    for e, lane, start, ln, ended, off in _episodes(lay):
        out[off:off + ln] = ref.returns_flat(reward[start:start + ln, lane:lane + 1], [ln], [0, ln], gamma)
    return out


def episode_return(reward, lay):
    reward = np.asarray(reward)
    out = np.zeros(len(lay["ep_lane"]), dtype=np.float64)
    for e, lane, start, ln, ended, off in _episodes(lay):
        out[e] = ref.episode_return(reward[start:start + ln, lane:lane + 1], [ln])[0]
    return out


def covered_cases(done, before, lay, reward, bootstrap):
    """Which of the lanes the issue lists a rollout holds (name -> bool)."""
    done = np.asarray(done) != 0
    before = np.asarray(before) != 0
    T, n = done.shape
    first, last = lay["lane_episode"][:-1], lay["lane_episode"][1:]
    rows = np.diff(lay["lane_row"])
    eps = last - first
    ended_all = np.array([lay["ep_ended"][a:b].all() for a, b in zip(first, last)])
    kept = kept_frames(done, before)
    len1_after_respawn = any(lay["ep_length"][e] == 1 and lay["ep_start"][e] >= 2 and
                             done[lay["ep_start"][e] - 2, lay["ep_lane"][e]] for e in range(len(lay["ep_lane"])))
    sticky = [i for i in range(n) if done[:, i].any() and not before[i] and done[done[:, i].argmax():, i].all()
              and done[:, i].argmax() < T - 2]
    open_eps = np.nonzero(lay["ep_ended"] == 0)[0]
    return {
        "done at frame 0": bool((done[0] & ~before).any()),
        "done at frame T-1, nothing open": bool((done[T - 1] & kept[T - 1] & ended_all).any()),
        "done at frame T-2": bool((done[T - 2] & kept[T - 2] & ~done[T - 1] & ended_all & (eps > 0)).any()),
        "done_before": bool((before & (rows > 0)).any()),
        "done_before and every frame done": bool((before & done.all(axis=0) & (rows == 0)).any()),
        "never done": bool((~before & ~done.any(axis=0) & (rows == T) & (eps == 1)).any()),
        "episode of length 1": bool(len1_after_respawn),
        "sticky lane": bool(sticky) and all(eps[i] == 1 for i in sticky),
        "three or more episodes": bool((eps >= 3).any()),
        "open with a bootstrap": bool(any(bootstrap[lay["ep_lane"][e]] != 0 and lay["ep_start"][e] > 0
                                          for e in open_eps)),
        "terminal rewards >= 500": bool((np.abs(reward[done & kept]) >= 500.0).all() and (done & kept).any()
                                        and (reward[done & kept] < 0).any() and (reward[done & kept] > 500.0).any()),
    }


normalize = ref.normalize
actions_f32 = ref.actions_f32
