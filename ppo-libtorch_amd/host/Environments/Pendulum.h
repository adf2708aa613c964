// Pendulum-v1 (gymnasium's classic_control/pendulum.py; the reference has no continuous-action env): the host-side class of PPO_ENV_PENDULUM, in the shape of
// MountainCar.h.  One real-valued action, the torque; step() takes the policy's RAW sample and the env clips its own copy to [-2, 2].
#pragma once
#include <tuple>
#include <vector>

#include "../Tensor.h"

class Pendulum {
  public:
    float max_speed, max_torque, dt, g, m, l;
    std::vector<float> low, high, state;   // state = {theta, theta_dot}; the observation is {cos theta, sin theta, theta_dot}
    int64_t episode_length;
    float episode_reward;

    explicit Pendulum(std::shared_ptr<ppo::Device> device = nullptr, int64_t seed = 1, int64_t env_index = 0);
    // {observation, reward, terminated (never), truncated (never: the algorithm counts max_episode_steps)}
    std::tuple<std::vector<float>, float, bool, bool> step(const std::vector<float>& action);
    std::vector<float> reset();            // the observation of the new state
    std::vector<float> observation() const { return m_obs; }

  protected:
    std::vector<float> randomUniform(float low, float high);   // {U(low, high), U(-1, 1)}

  private:
    std::shared_ptr<ppo::Device> m_device;
    int64_t m_seed, m_env_index, m_resets = 0;
    std::vector<float> m_obs;
};
