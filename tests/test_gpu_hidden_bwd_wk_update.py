"""PPO.update() of the wide stack [512, 256, 128] with the fused backward of its 512 -> 256 layer
(fused_mlp.hidden_bwd_pair_wk) and with the two separate launches (RSLRL_HIDDEN_BWD_WK=0's path) on one storage: one
launch per network and mini-batch (train_backward), the same learning-rate trace, loss statistics rtol 1e-4, parameters
within fp32 accumulation-order noise (tests/test_gpu_hidden_bwd_kn_update.py's set-up and tolerances).  Observation
width 235 puts a ragged first layer in front of the wide layer."""

import numpy as np
import pytest
import torch

from rsl_rl_amd.networks import fused_mlp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("O", [48, 235])
def test_update_with_hidden_bwd_wk(O, cuda_device, monkeypatch):
    from rsl_rl_amd.algorithms import PPO
    from rsl_rl_amd.modules import ActorCritic

    dev = cuda_device
    dims = [512, 256, 128]
    T, N, A = 8, 2048, 12
    epochs, batches = 2, 4
    obs0 = {"policy": torch.zeros(N, O)}
    groups = {"policy": ["policy"], "critic": ["policy"]}
    rng = np.random.default_rng(9)
    data = {k: rng.standard_normal(s).astype(np.float32) for k, s in
            (("obs", (T, N, O)), ("rewards", (T, N, 1)), ("values", (T, N, 1)), ("logp", (T, N, 1)),
             ("mu", (T, N, A)), ("actions", (T, N, A)), ("last", (N, O)))}
    results = []
    for use in (True, False):
        monkeypatch.setattr(fused_mlp, "_HIDDEN_BWD_WK", use)
        calls = []
        real = fused_mlp.hidden_bwd_pair_wk
        monkeypatch.setattr(fused_mlp, "hidden_bwd_pair_wk", lambda *a, **k: calls.append(len(a[0])) or real(*a, **k))
        torch.manual_seed(0)
        pol = ActorCritic(obs0, groups, A, actor_hidden_dims=dims, critic_hidden_dims=dims)
        alg = PPO(pol, num_learning_epochs=epochs, num_mini_batches=batches, device=dev, desired_kl=0.01)
        alg.init_storage("rl", N, T, obs0, [A])
        st = alg.storage
        st.observations["policy"].copy_(torch.from_numpy(data["obs"]))
        st.rewards.copy_(torch.from_numpy(data["rewards"]))
        st.values.copy_(torch.from_numpy(data["values"]))
        st.actions_log_prob.copy_(torch.from_numpy(data["logp"]) - 10.0)
        st.mu.copy_(torch.from_numpy(data["mu"]) * 0.1)
        st.sigma.copy_(torch.ones(T, N, A))
        st.actions.copy_(torch.from_numpy(data["actions"]))
        st.dones.zero_()
        st.step = T
        with torch.inference_mode():
            alg.compute_returns({"policy": torch.from_numpy(data["last"]).to(dev)})
        st.perm_generator = torch.Generator().manual_seed(1)
        loss = alg.update()
        # one single-problem launch per network and mini-batch
        assert calls == ([1] * (2 * batches * epochs) if use else [])
        monkeypatch.setattr(fused_mlp, "hidden_bwd_pair_wk", real)
        results.append((loss, alg.learning_rate, {k: v.detach().clone() for k, v in pol.state_dict().items()}))
    (l1, lr1, p1), (l0, lr0, p0) = results
    assert lr1 == lr0
    for k in l0:
        assert np.isclose(l1[k], l0[k], rtol=1e-4, atol=1e-7), k
    for k in p0:
        assert torch.allclose(p1[k], p0[k], rtol=1e-4, atol=2e-6), k
