"""The row-wise attend-and-excite update (udt_aae_row_update_f32, include/udt_kernels.h) restated in plain torch, and the analytic toy
loss of tests/golden/aae_rows_golden.npz — shared by the golden's generator and the tests.  No GPU, no library.

The rule, for row b of a batch with a = (state_in[0, b] != 0):
    a:      x[b] <- fma(-alpha, grad[b], x[b])                         (one rounding; float64 product + sum rounded once, see ``fma32``)
    not a:  x[b] untouched; grad[b] and loss[b] are not looked at
    it = state_in[1, b] + a
    state_out[0, b] = a and iter_enabled and not (loss[b] <= thres) and not (it > max_iter)       (reference sampling.py:249)
    state_out[1, b] = it
    n_active = sum_b state_out[0, b]
"""
import torch


def fma32(a: float, y: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """fp32 fma(a, y, x) on fp32 tensors: the product of two fp32 values is exact in float64 (48 significant bits), the float64 sum
    carries <= 2^-53 relative error before the final rounding to fp32 — correctly rounded except on a double-rounding tie, which needs
    the 29 bits below fp32's last place to be exactly 1000...0 after the first rounding: not met by the data of these tests (the tests
    that ask for bit equality compare against the library's own udt_axpy_f32, not against this)"""
    a32 = float(torch.tensor(a, dtype=torch.float32))
    return (a32 * y.double() + x.double()).float()


def row_update(x, grad, loss, state_in, alpha, thres, iter_enabled, max_iter):
    """-> (x_new fp32 [B, ...], state_out int32 [2, B], n_active int); inputs are not modified.  Frozen rows' grad / loss are never
    read (they may hold NaN)."""
    B = x.shape[0]
    x_new = x.clone()
    state_out = torch.zeros((2, B), dtype=torch.int32)
    for b in range(B):
        a = int(state_in[0, b]) != 0
        it = int(state_in[1, b]) + int(a)
        nxt = False
        if a:
            x_new[b] = fma32(-float(alpha), grad[b], x[b])
            nxt = bool(iter_enabled) and not (float(loss[b]) <= float(thres)) and not (it > int(max_iter))
        state_out[0, b] = int(nxt)
        state_out[1, b] = it
    return x_new, state_out, int(state_out[0].sum())


def row_loop(x0, evaluate, alpha, thres, iter_enabled, max_iter, update=row_update):
    """the row-wise loop on a batch: evaluate(x) -> (loss [B], grad like x); -> (x_final, counts int32 [B], evaluations, losses list)"""
    B = x0.shape[0]
    x = x0.clone()
    state = torch.zeros((2, B), dtype=torch.int32)
    state[0] = 1
    evals, losses = 0, []
    while True:
        loss, grad = evaluate(x)
        losses.append(loss.clone())
        x, state, n_active = update(x, grad, loss, state, alpha, thres, iter_enabled, max_iter)
        evals += 1
        if n_active == 0:
            break
    return x, state[1].clone(), evals, losses


# ------------------------------------------------------------------------------------------------ the golden's toy loss
TOY_FREQ, TOY_RIPPLE = 0.7, 0.05


def toy_loss(x, w, t, c):
    """smooth per-sample loss of x [B, 4, 8, 8]: c_b + mean_i (w_bi (x_bi - t_bi)^2 / 2 + TOY_RIPPLE cos(TOY_FREQ x_bi)) -> [B]"""
    d = x - t
    return c + (0.5 * w * d * d + TOY_RIPPLE * torch.cos(TOY_FREQ * x)).flatten(1).mean(1)


def toy_loss_grad(x, w, t, c):
    """(toy_loss, its gradient written out: (w (x - t) - TOY_RIPPLE TOY_FREQ sin(TOY_FREQ x)) / n)"""
    n = x[0].numel()
    return toy_loss(x, w, t, c), (w * (x - t) - (TOY_RIPPLE * TOY_FREQ) * torch.sin(TOY_FREQ * x)) / n


def displacement_bound(k, alpha, x0, x_final, g0):
    """max |x_final - reference x_final| after k updates of the toy, from the arithmetic alone.  Per update the rule rounds once
    (the fma: 2^-24 |x'|); the reference rounds alpha * grad and the subtraction (2^-24 (|alpha g| + |x'|)); the two gradients (autograd
    against the written-out form) are each a handful of fp32 operations on values of the size of g: <= 4 roundings a side, 2^-24 *
    8 |alpha g| together.  Sum: 2^-24 (2 |x'| + 9 |alpha g|) <= 11 * 2^-24 M <= 2^-20 M per update, with M the largest of |x| and
    |alpha g| along the run (|x - t| and with it |g| shrink under the toy's updates, so the first gradient and the end points bound
    them).  The update map x -> x - alpha grad(x) is non-expansive for the toy (alpha f'' in [0, 2): w alpha / n <= 0.4 and the
    ripple's curvature alpha * 0.0245 / n is below 0.01), so the per-update errors add and do not grow: k * 2^-20 * M."""
    M = max(float(x0.abs().max()), float(x_final.abs().max()), float(alpha) * float(g0.abs().max()))
    return k * 2.0 ** -20 * M
