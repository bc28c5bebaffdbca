"""MI355X-native Koopman-MPC window engine.

Drop-in for the reference's per-window hot path (yli421/koopman-mpc-portfolio-rebalancing):
``MPCConfig`` / ``solve_mpc_log_utility`` (mpc.py) and ``BacktestConfig`` / ``Strategy`` /
``BuyAndHoldStrategy`` / ``KoopmanMPCStrategy`` / ``run_backtest`` / ``calculate_metrics``
(backtest.py), executed by hand-written gfx950 kernels in libkmpc.so (C ABI: include/kmpc.h).
"""
from .mpc import (MPCConfig, gross_returns, log_utility_value_batched, solve_mpc_log_utility,  # noqa: F401
                  solve_mpc_log_utility_batched, solve_mpc_mean_variance, solve_mpc_mean_variance_banded,
                  solve_mpc_mean_variance_banded_batched, solve_mpc_mean_variance_batched)
from .koopman import DeviceKoopman, KoopmanModelSpec, standardize_panel  # noqa: F401
from .backtest import (BacktestConfig, BuyAndHoldStrategy, KoopmanMPCStrategy, Strategy,  # noqa: F401
                       calculate_metrics, run_backtest, run_backtest_lockstep, run_backtest_sweep,
                       sweep_backtest)
from .baselines import (KoopmanMVStrategy, run_koopman_mv_lockstep, run_koopman_mv_sweep,  # noqa: F401
                        run_markowitz_lockstep, run_markowitz_sweep, sweep_backtest_koopman_mv,
                        sweep_backtest_markowitz)

__version__ = "0.7.0"
