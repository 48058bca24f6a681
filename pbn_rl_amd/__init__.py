"""pbn_rl_amd -- MI355X-native batched PBN environment (gym-PBN step hot path).

Public surface:
  network.Network / load_network     ISPL + logic-function compiler
  attractors                         attractor fixtures / discovery
  spec.EnvSpec                       one environment definition (C descriptor)
  vector_env.VectorPBNEnv            batched envs in HBM, stepped by libpbn_env.so
  env.PBNEnv / make                  scalar gym-style facade (drop-in under train_BDQ.py)
  evaluate.evaluate_control          source -> target control evaluation of a trained agent
  ddqn.DQN / DDQNLearner             the reference's DDQN / DDQN-PER agent over the batched envs
  ssd.compute_ssd_hist               steady-state distribution (dense bins, or sparse=True: any width)
  state_table.StateTable             visited-state counts in a device hash table
  episode_stats.EpisodeStats         episode returns, lengths and per-pair misses kept on the device
  curriculum.Curriculum              restarts weighted by the per-pair statistics (rework_probas), on the device
  checkpoint / learner.save, load    a training run written out and resumed bit-equal (tools/train.py)
"""
__version__ = "0.1.0"
