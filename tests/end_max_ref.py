"""TEST-ONLY helpers of the end_mode='max' training path (tests/test_end_max_cpu.py, tests/test_end_max_gpu.py):

* ``EndMaxOps``: tests/fake_ops.py::TorchOps plus the two operators of the arg-max backward (mmmot_segment_argmax,
  mmmot_pair_expand_max_bwd of include/mmmot_hip.h) in executable-specification form;
* ``reference_grads``: tests/test_backward_cpu.py::reference_grads with the oracle's ``end_mode``;
* ``top_two_gaps``: how far the largest value of every maximum is from the runner-up, on the float64 restatement - the
  condition under which an fp32 implementation must pick the same row as float64.
"""
import torch
import torch.nn.functional as Fn

from fake_ops import TorchOps
from oracle import restatement as R


class EndMaxOps(TorchOps):
    name = 'torch-emulation+end-max'

    def segment_argmax(self, X, C, segs, idx, sc=None, sh=None, relu=False, use_group=True):
        """idx[s][c] = the FIRST t of segment s that attains max_t a(t); a(t) is what ``segment_mean`` above pools (same
        expression, same dtype), so a(idx) is the value ``segment_mean(take_max=True)`` writes.  A scan in increasing t
        with a strict >: the rule of torch's max(dim)."""
        for s in range(segs.n):
            st, cnt, stride = int(segs.h_start[s]), int(segs.h_count[s]), int(segs.h_stride[s])
            rows = X[st:st + (cnt - 1) * stride + 1:stride, :C]
            if sc is not None:
                g = int(segs.h_group[s]) if use_group else 0
                rows = rows * sc[g, :C] + sh[g, :C]
            if relu:
                rows = torch.relu(rows)
            best, bi = rows[0].clone(), torch.zeros(C, dtype=torch.int32)
            for t in range(1, cnt):
                m = rows[t] > best
                best = torch.where(m, rows[t], best)
                bi[m] = t
            idx[s, :C] = bi

    def pair_expand_max_bwd(self, dV, idx, dA, C, tiles, row0, gN, gM, vrow0):
        """dA[(g,i,j)] = (idx[v0 + j] == i ? dV[v0 + j] : 0) + (idx[v0 + M + i] == j ? dV[v0 + M + i] : 0): selection, then
        ONE add in dV's precision, new + end"""
        for g in range(row0.numel()):
            N, M, r0, v0 = int(gN[g]), int(gM[g]), int(row0[g]), int(vrow0[g])
            new, end = dV[v0:v0 + M, :C], dV[v0 + M:v0 + M + N, :C]
            kn, ke = idx[v0:v0 + M, :C].long(), idx[v0 + M:v0 + M + N, :C].long()
            i, j = torch.arange(N).view(N, 1, 1), torch.arange(M).view(1, M, 1)
            zero = torch.zeros((), dtype=dV.dtype)
            a = torch.where(kn.unsqueeze(0) == i, new.unsqueeze(0), zero)   # [N][M][C]
            b = torch.where(ke.unsqueeze(1) == j, end.unsqueeze(1), zero)
            dA[r0:r0 + N * M, :C] = (a + b).reshape(N * M, C).to(dA.dtype)


def _pairs(samples):
    """(column offset of the previous frame, N, M) of every frame pair of a batch of samples (lists of frame counts)"""
    off = 0
    for counts in samples:
        d0 = off
        for p in range(len(counts) - 1):
            yield d0, counts[p], counts[p + 1]
            d0 += counts[p]
        off += sum(counts)


def reference_grads(model, samples, F, op, sm, w_link, w_new, w_end, end_mode='max'):
    """float64 autograd through the oracle's pairwise block with ``end_mode``; F [nR, Lt, 512] (ours) <-> [nR, 512, L]
    (reference).  Same loss as tests/test_backward_cpu.py::reference_grads: every score times a fixed weight."""
    sd = {k: v.detach().double().clone().requires_grad_(k.startswith('w_link.')) for k, v in model.state_dict().items()}
    Fd = F.detach().double().clone().requires_grad_(True)
    F3 = Fd.permute(0, 2, 1)
    loss, lo = 0.0, 0
    for d0, N, M in _pairs(samples):
        logit, nw, en = R.affinity(F3[:, :, d0:d0 + N], F3[:, :, d0 + N:d0 + N + M], sd, op, end_mode=end_mode)
        lk = R.softmax_mode(logit, sm).squeeze(1)
        n = lk.numel()
        loss = loss + (lk.reshape(-1) * w_link[lo:lo + n].double()).sum()
        lo += n
        loss = loss + (nw * w_new[:, d0 + N:d0 + N + M].double()).sum() + (en * w_end[:, d0:d0 + N].double()).sum()
    loss.backward()
    return Fd.grad, {k: v.grad for k, v in sd.items() if k.startswith('w_link.')}


def conv0_activations(model_state_dict, F, samples, op):
    """relu(gn(conv0(pairwise))) of every frame pair, nR x 512 x N x M each: what the new / end pool reduces (float64
    restatement of reference modules/new_end.py:66-68)"""
    sd = {k: v.detach().double() for k, v in model_state_dict.items()}
    F3 = F.detach().double().permute(0, 2, 1)
    p = 'w_link.w_new_end.'
    for d0, N, M in _pairs(samples):
        x = R.pairwise(F3[:, :, d0:d0 + N], F3[:, :, d0 + N:d0 + N + M], op)
        yield Fn.relu(R._gn(Fn.conv2d(x, sd[p + 'conv0.0.weight'], sd[p + 'conv0.0.bias']), sd, p + 'conv0.1', 1))


def conv0_rows(model_state_dict, F, samples, op):
    """the same tensor in the plan's pair-row order [sum nR*N*M][512] (group = pair * nR + modality row, row = i * M + j)"""
    return torch.cat([x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]) for x in conv0_activations(model_state_dict, F, samples, op)])


def top_two_gaps(model_state_dict, F, samples, op):
    """Per (new / end vector, channel) with a positive maximum and at least two rows: (largest - second largest) of
    relu(gn(conv0(pairwise))) over the pooled axis, divided by the tensor's maximum; float64 restatement.  Returns the
    1-D tensor of all of them (its minimum decides whether float64 and fp32 must agree on every arg-max)."""
    gaps = []
    for x in conv0_activations(model_state_dict, F, samples, op):
        scale = x.max().item()
        for dim in (-2, -1):  # new vectors pool the previous frame's axis, end vectors the current one's
            if x.shape[dim] < 2:
                continue
            top = x.topk(2, dim=dim)[0]
            hi, second = top.select(dim, 0), top.select(dim, 1)
            gaps.append(((hi - second)[hi > 0] / scale).reshape(-1))
    return torch.cat(gaps) if gaps else torch.full((1,), float('inf'), dtype=torch.float64)
