// MountainCarContinuous-v0 (gymnasium's classic_control/continuous_mountain_car.py; the reference has only the discrete MountainCar): the host-side class of
// PPO_ENV_MOUNTAINCAR_CONTINUOUS, in the shape of Pendulum.h.  One real-valued action, the force; step() takes the policy's RAW sample, the env clips its own
// copy to [-1, 1] and charges the raw one (0.1 a^2).  The observation is the state.
#pragma once
#include <tuple>
#include <vector>

#include "../Tensor.h"

class MountainCarContinuous {
  public:
    float min_action, max_action, min_position, max_position, max_speed, goal_position, goal_velocity, power, gravity;
    std::vector<float> low, high, state;   // state = {position, velocity} = the observation
    int64_t episode_length;
    float episode_reward;

    explicit MountainCarContinuous(std::shared_ptr<ppo::Device> device = nullptr, int64_t seed = 1, int64_t env_index = 0);
    // {observation, reward, terminated (the goal reached with a velocity >= 0), truncated (never: the algorithm counts max_episode_steps)}
    std::tuple<std::vector<float>, float, bool, bool> step(const std::vector<float>& action);
    std::vector<float> reset();            // the observation of the new state
    std::vector<float> observation() const { return state; }

  protected:
    std::vector<float> randomUniform(float low, float high);   // {U(low, high), 0}

  private:
    std::shared_ptr<ppo::Device> m_device;
    int64_t m_seed, m_env_index, m_resets = 0;
};
