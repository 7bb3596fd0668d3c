"""Fits the initializer network to recorded demonstrations: nn_trainer/nn_trainer.py:175-273 (build_dataset, train_net,
test_pth_model) on the arrays of `record.DemoRecorder.training_tensors()` instead of a CSV and a folder of PNGs."""
import numpy as np


def train_initializer(inputs, labels, net=None, epochs=5, batch_size=2, lr=1e-3, train_fraction=0.8, seed=42, device=None,
                      train_backbone=False):
    """inputs (n, H * W + 24) float32 (process_input_np's layout), labels (n, 9) float32 (body-frame waypoints, then
    durations).  As the reference: torch.manual_seed(seed), then the network (net None: PlannerNet() at 640 x 480),
    random_split at int(train_fraction * n), batches of `batch_size` in the split's order without shuffling, Adam(lr) on
    MSELoss(reduction='mean'), an epoch's loss the mean over its batches, and at the end the held-out MSE, averaged
    over batches, with the network in eval mode.

    The reference freezes an ImageNet-pretrained ResNet-18 and trains only the stem and the fc it replaces (:113-122)
    besides the dense branches.  Pretrained weights are not available here: the backbone is frozen at its seeded random
    initialisation instead (a fixed random feature map under the trainable stem and fc), unless train_backbone=True
    trains all of it.  The flags are put back as they were afterwards.

    device None: the GPU when there is one.  Returns (net, losses: one float per epoch, held_out: float)."""
    import torch
    from . import initializer as ini

    torch.manual_seed(int(seed))
    if net is None:
        net = ini.PlannerNet()
    x = torch.as_tensor(np.ascontiguousarray(inputs, dtype=np.float32))
    y = torch.as_tensor(np.ascontiguousarray(labels, dtype=np.float32))
    n = x.shape[0]
    if x.ndim != 2 or y.ndim != 2 or y.shape[0] != n or x.shape[1] != net.img_height * net.img_width + ini.MOTION_INPUT_SIZE:
        raise ValueError("train_initializer: inputs (n, H * W + 24) for the network's image size, labels (n, outputs)")
    n_train = int(train_fraction * n)
    if n_train < 1 or n - n_train < 1:
        raise ValueError("train_initializer: both parts of the split need a row")
    dev = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    train_set, test_set = torch.utils.data.random_split(torch.utils.data.TensorDataset(x, y), [n_train, n - n_train],
                                                        generator=torch.Generator().manual_seed(int(seed)))
    train_idx, test_idx = torch.as_tensor(train_set.indices), torch.as_tensor(test_set.indices)

    def batches(idx):
        for k0 in range(0, idx.shape[0], int(batch_size)):
            pick = idx[k0:k0 + int(batch_size)]
            yield x[pick].to(dev), y[pick].to(dev)

    was = {name: p.requires_grad for name, p in net.named_parameters()}
    for name, p in net.img_backbone.named_parameters():
        p.requires_grad = bool(train_backbone) or name.startswith("conv1.") or name.startswith("fc.")
    net = net.to(dev)
    criterion = torch.nn.MSELoss(reduction="mean")
    optimizer = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=lr)
    losses = []
    net.train()
    for _ in range(int(epochs)):
        running, count = 0.0, 0
        for xb, yb in batches(train_idx):
            optimizer.zero_grad()
            loss = criterion(net(xb), yb)
            loss.backward()
            optimizer.step()
            running += loss.item()
            count += 1
        losses.append(running / count)
    net.eval()
    with torch.no_grad():
        total, count = 0.0, 0
        for xb, yb in batches(test_idx):
            total += criterion(net(xb), yb).item()
            count += 1
    for name, p in net.named_parameters():
        p.requires_grad = was[name]
    return net, losses, total / count
